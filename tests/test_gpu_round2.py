"""GPU tests added in round 2 (all through the C ABI via alignq_amd.ops / the Python mirror):
general corr(x, y); the stand-alone `cdf` module; idempotent reduce+loss; lazy batch-norm link safety; capture guards
(momentum buffers, off-shape batches); the Office / DANN iteration at value level against the reference fixture G10."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-5


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


# ------------------------------------------------------------------------------------------------ corr(x, y), y != x
@pytest.mark.parametrize("fname,tree,cases", [("g4b_corr_xy_noeps", "admm", 3), ("g4b_corr_xy_eps", "office", 2)])
def test_general_corr_xy_vs_reference_and_oracle(dev, fname, tree, cases):
    import alignq_amd.cdf_alignment_admm as A
    import alignq_amd.office as Off
    ns, eps = (A, 0.0) if tree == "admm" else (Off, 1e-5)
    g = load_golden(fname)
    for ci in range(cases):
        x = cu(g[f"x_c{ci}"], dev).requires_grad_(True)
        y = cu(g[f"y_c{ci}"], dev).requires_grad_(True)
        G = ns.corr(x, y)
        G.backward(cu(g[f"dG_c{ci}"], dev))
        np.testing.assert_allclose(npy(G), g[f"G_c{ci}"], atol=TOL)
        np.testing.assert_allclose(npy(x.grad), g[f"dx_c{ci}"], atol=TOL, rtol=1e-4)
        np.testing.assert_allclose(npy(y.grad), g[f"dy_c{ci}"], atol=TOL, rtol=1e-4)
        Go = O.corr_xy_fwd(g[f"x_c{ci}"], g[f"y_c{ci}"], eps)
        np.testing.assert_allclose(npy(G), Go, atol=2e-6)
    # ragged shapes against the oracle; x alone needing a gradient; corr(x, x.clone()) == the SYRK path
    rng = np.random.default_rng(0)
    for B, F in ((2, 64), (33, 70), (128, 4100), (100, 31)):
        x0 = (rng.standard_normal((B, F)) * 0.9 + 0.2).astype(np.float32)
        y0 = (rng.standard_normal((B, F)) * 1.4 - 0.1).astype(np.float32)
        dG = rng.standard_normal((B, B)).astype(np.float32)
        x, y = cu(x0, dev).requires_grad_(True), cu(y0, dev)
        G = A.corr(x, y)
        G.backward(cu(dG, dev))
        np.testing.assert_allclose(npy(G), O.corr_xy_fwd(x0, y0), atol=TOL)
        dxo, _ = O.corr_xy_bwd(dG, x0, y0)
        rho = 1.0 / x0.std(0, ddof=1)
        np.testing.assert_allclose(npy(x.grad), dxo, atol=TOL * max(1.0, float(rho.max()) / 10), rtol=1e-4)
        if B > 2:
            xs = cu(x0, dev)
            # exact fp32 vs the split-bf16 SYRK (2^-16 relative per product; averages out as 1/sqrt(F), F = 31 is the worst here)
            np.testing.assert_allclose(npy(A.corr(xs, xs.clone())), npy(A.corr(xs, xs)), atol=2e-5)


# ------------------------------------------------------------------------------------------------ cdf nn.Module (R2)
def test_cdf_module_vs_reference(dev):
    """`cdf(m, s, quant_src).forward(tensor) -> (cdf, pdf)` used stand-alone (ADMM tree model/quantization.py:41-59): values
    (k=32 path of alignq_weight_quant_fwd, the 'a' scaling by act_range) and the gradient attached to the first output."""
    import alignq_amd.cdf_alignment_admm as A
    g = load_golden("g11_cdf_module_admm")
    for src in ("a", "w"):
        v = cu(g["v"], dev).requires_grad_(True)
        mod = A.cdf(torch.tensor(float(g[f"m_{src}"])), torch.tensor(float(g[f"s_{src}"])), src)
        c, pdf = mod(v)
        c.backward(cu(g["gc"], dev))
        np.testing.assert_allclose(npy(c), g[f"cdf_{src}"], atol=1e-6)
        np.testing.assert_allclose(npy(pdf), g[f"pdf_{src}"], atol=1e-6, rtol=1e-5)
        np.testing.assert_allclose(npy(v.grad), g[f"dv_{src}"], atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("tree,fname", [("admm", "g11b_cdf_live_stats_admm"), ("cdf", "g11b_cdf_live_stats_cdfonly")])
def test_cdf_module_with_live_statistics_vs_reference(dev, tree, fname):
    """Round 5: `cdf(m, s, src)` with m and s as tensors of the autograd graph - the reference's own use is
    cdf(torch.mean(x), torch.std(x), 'w')(x) (ADMM tree model/quantization.py:78, CDF tree :70).  Gradients of BOTH outputs w.r.t.
    the tensor, m and s (alignq_cdf_bwd) vs fixture G11b, and dW of the composed form through mean / std."""
    import importlib
    A = importlib.import_module("alignq_amd.cdf_alignment_admm" if tree == "admm" else "alignq_amd.cdf_alignment")
    g = load_golden(fname)
    gc, gp = cu(g["gc"], dev), cu(g["gp"], dev)
    for src in ("w", "a"):
        v = cu(g["v"], dev).requires_grad_(True)
        m = torch.tensor(float(g[f"m_{src}"]), device=dev, requires_grad=True)
        s = torch.tensor(float(g[f"s_{src}"]), device=dev, requires_grad=True)
        c, pdf = A.cdf(m, s, src)(v)
        torch.autograd.backward([c, pdf], [gc, gp])
        np.testing.assert_allclose(npy(c), g[f"cdf_{src}"], atol=1e-6)
        np.testing.assert_allclose(npy(pdf), g[f"pdf_{src}"], atol=1e-6, rtol=1e-5)
        np.testing.assert_allclose(npy(v.grad), g[f"dv_{src}"], atol=2e-6, rtol=1e-5)
        np.testing.assert_allclose(float(m.grad), float(g[f"dm_{src}"]), rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(float(s.grad), float(g[f"ds_{src}"]), rtol=2e-5, atol=2e-5)
    w = cu(g["v"], dev).requires_grad_(True)
    c, pdf = A.cdf(torch.mean(w), torch.std(w), "w")(w)
    c.backward(gc)
    np.testing.assert_allclose(npy(c), g["cdf_ms"], atol=1e-6)
    np.testing.assert_allclose(npy(w.grad), g["dW_ms"], atol=2e-6, rtol=1e-5)
    # constants still work (python floats / tensors without a graph): the gradient reaches the tensor only
    v = cu(g["v"], dev).requires_grad_(True)
    c, pdf = A.cdf(0.07, 0.6, "w")(v)
    c.backward(gc)
    np.testing.assert_allclose(npy(v.grad), npy(gc * pdf.detach()) * (1.0 if tree == "admm" else 0.5), atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ reduce + loss hand-off
@pytest.mark.parametrize("B,F", [(128, 16384), (100, 4096), (28, 6272)])
def test_reduce_loss_is_idempotent_and_matches_the_oracle(dev, B, F):
    """alignq_site_reduce_loss: the last-arriver epilogue re-arms its ticket, so reducing the same workspace again (20x)
    gives the same D bits and the same loss every time; loss == the oracle's ADMM loss of that D."""
    from alignq_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(B)
    x = cu((rng.standard_normal((B, F)) * 1.2).astype(np.float32), dev)
    A0 = (rng.standard_normal((128, 128)) * 0.05).astype(np.float32)
    G0 = (rng.standard_normal((128, 128)) * 0.05).astype(np.float32)
    A, Gm = cu(A0, dev), cu(G0, dev)
    xq = torch.empty_like(x)
    stats = torch.empty(4, F, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.alignq_site_ws_bytes(B, F), dtype=torch.uint8, device=dev)
    st = L.stream_ptr()
    L.check(lib.alignq_site_partials(L.ptr(x), B, F, 8, 2.0, 0.0, L.ptr(xq), L.ptr(stats), L.ptr(ws), st), "partials")
    outs = []
    for _ in range(20):
        D = torch.zeros(B, B, dtype=torch.float32, device=dev)
        scal = torch.full((4,), -1.0, dtype=torch.float32, device=dev)
        L.check(lib.alignq_site_reduce_loss(L.ptr(ws), B, F, L.ptr(D), L.ptr(A), L.ptr(Gm), 128, 0.2, 0.3, L.ptr(scal), st),
                "reduce_loss")
        outs.append((npy(D), npy(scal)))
    for D, scal in outs[1:]:
        assert np.array_equal(D, outs[0][0]) and np.array_equal(scal, outs[0][1])
    loss_o, _, _, _ = O.admm_loss(outs[0][0], A0, G0, 0.2, 0.3)
    np.testing.assert_allclose(outs[0][1][0], loss_o, atol=1e-6)


# ------------------------------------------------------------------------------------------------ lazy BN link safety
def _conv_bn_site(dev, k=8, B=128, C=16, H=32, seed=0):
    import alignq_amd.cdf_alignment_admm as A
    from alignq_amd import config
    config.args.bitW = config.args.abitW = k
    torch.manual_seed(seed)
    n = 2 ** k - 1
    cl = torch.channels_last
    x = (torch.randn(B, C, H, H, device=dev) * 1.1).contiguous(memory_format=cl).requires_grad_(True)
    w = (torch.round(torch.tanh(torch.randn(C, C, 3, 3)) * n) / n).to(dev).contiguous(memory_format=cl).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    admm = A.ADMM(128).to(dev)
    act = A.activation_quantize_fn(k, "second", admm)
    gq = torch.randn(B, C, H, H, device=dev).contiguous(memory_format=cl) * 0.01
    return x, w, bn, act, gq


class _Flush(torch.autograd.Function):        # stands in for the weight quantiser's backward (flushes deferred wgrads)
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        from alignq_amd.fused import active_wgrads
        if active_wgrads() is not None:
            active_wgrads().flush()
        return g


def test_lazy_bn_gradient_altered_on_the_way_raises_instead_of_being_used_as_dz(dev):
    """a tensor hook on the convolution output z stands between BNSiteFn.backward and the convolution's backward;
    the gradient that arrives is no longer the posted lazy record's tensor.  The consumer must refuse it (round 1 keyed the
    record by data_ptr and would silently have treated the BN-output gradient as dz)."""
    from alignq_amd import ops
    from alignq_amd.fused import DeferredWgrads, bn_site
    x, w, bn, act, gq = _conv_bn_site(dev)
    z = ops.QConv3x3Fn.apply_with_stats(x, _Flush.apply(w), 8)
    z.register_hook(lambda g: g * 1.0)                  # returns a NEW tensor
    xq, loss = bn_site(bn, act, z, relu=True)
    with pytest.raises(RuntimeError, match="lazy batch-norm gradient"):
        with DeferredWgrads(fresh_grads=True):
            (loss + (xq * gq).sum()).backward()


def test_lazy_bn_with_existing_bn_grads_takes_the_materialised_path(dev):
    """fresh_grads is checked, not trusted: with a pre-existing bn.weight.grad the in-kernel form (which fills dgamma after
    autograd adopted it) must not be used; the result equals the plain path accumulated onto the old gradient."""
    from alignq_amd import ops
    from alignq_amd.fused import DeferredWgrads, bn_site
    res = []
    for pre in (False, True):
        x, w, bn, act, gq = _conv_bn_site(dev, seed=3)
        if pre:
            bn.weight.grad = torch.full_like(bn.weight, 0.5)
            bn.bias.grad = torch.full_like(bn.bias, -0.25)
        z = ops.QConv3x3Fn.apply_with_stats(x, _Flush.apply(w), 8)
        xq, loss = bn_site(bn, act, z, relu=True)
        with DeferredWgrads(fresh_grads=True) as wg:
            (loss + (xq * gq).sum()).backward()
            wg.flush()
        torch.cuda.synchronize()
        res.append((npy(bn.weight.grad), npy(bn.bias.grad), npy(x.grad), npy(w.grad)))
    (dg0, db0, dx0, dw0), (dg1, db1, dx1, dw1) = res
    np.testing.assert_allclose(dg1, dg0 + 0.5, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(db1, db0 - 0.25, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dx1, dx0, rtol=1e-4, atol=1e-5 * float(np.abs(dx0).max()))
    np.testing.assert_allclose(dw1, dw0, rtol=1e-4, atol=1e-5 * float(np.abs(dw0).max()))


# ------------------------------------------------------------------------------------------------ capture guards
def _tiny_step(dev, batch=72, **kw):
    from alignq_amd import config
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    from alignq_amd.train_step import TrainStep
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = batch
    torch.manual_seed(0)
    net = PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 4, 4, "second", 10).to(dev).train()
    return net, TrainStep(net, channels_last=True, qconv=True, **kw)


def _tiny_office_step(dev, batch=6):
    """OfficeTrainStep on the tiny DANN of fixture G10 (test_office_tiny_dann_two_iterations_vs_reference)."""
    from alignq_amd import config
    from alignq_amd.resnet_office import DANN, Bottleneck, ResNet
    from alignq_amd.train_step import OfficeTrainStep
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = batch
    torch.manual_seed(0)
    net = DANN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, "aligned").to(dev).train()
    return net, OfficeTrainStep(net, lr=0.004, channels_last=True)


@pytest.mark.parametrize("tree", ["cifar", "office"])
def test_capture_without_momentum_buffers_is_refused(dev, tree):
    """capture(warmup=0) on a fresh step would bake first=1 into the graph (buf = grad on every replay): the CIFAR
    TrainStep and the Office / DANN OfficeTrainStep alike."""
    from alignq_amd import config
    try:
        if tree == "cifar":
            net, step = _tiny_step(dev)
            inputs = (torch.randn(72, 3, 32, 32, device=dev), torch.randint(0, 10, (72,), device=dev))
        else:
            net, step = _tiny_office_step(dev)
            inputs = (torch.randn(6, 3, 64, 64, device=dev), torch.randint(0, 31, (6,), device=dev),
                      torch.randn(6, 3, 64, 64, device=dev))
        with pytest.raises(RuntimeError, match="momentum buffer"):
            step.capture(*inputs, warmup=0)
        step.capture(*inputs, warmup=1)                    # one eager step creates them: fine
        step(*inputs)
        torch.cuda.synchronize()
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100


def test_captured_step_runs_an_off_shape_batch_eagerly_and_keeps_its_graph(dev):
    """the reference's last CIFAR batch is short.  A captured TrainStep must run it eagerly (same
    result as an un-captured twin) and afterwards replay its graph as before (p.grad / ADMM.D name the graph's tensors)."""
    from alignq_amd import config
    try:
        x = torch.randn(72, 3, 32, 32, device=dev)
        y = torch.randint(0, 10, (72,), device=dev)
        xs, ys = x[:40].clone(), y[:40].clone()
        net_a, step_a = _tiny_step(dev)
        net_b, step_b = _tiny_step(dev)
        step_a.capture(x, y, warmup=2)
        for _ in range(2):
            step_b(x, y)
        seq = [(x, y), (xs, ys), (x, y), (x, y)]
        for xi, yi in seq:
            la, cea, _ = step_a(xi, yi)
            lb, ceb, _ = step_b(xi, yi)
            torch.cuda.synchronize()
            assert la.shape[0] == xi.shape[0]
            np.testing.assert_allclose(float(cea), float(ceb), rtol=2e-2, atol=1e-2)
        g_graph = net_a.logit.weight.grad
        step_a(x, y)
        assert net_a.logit.weight.grad is g_graph                      # the graph's gradient tensor is back in place
        assert tuple(step_a.admms[0].D.shape) == (72, 72)
        for (n, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
            if pa.numel() >= 64 and "alterD" not in n and "gamma" not in n:
                a, b = pa.detach().flatten(), pb.detach().flatten()
                cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
                assert cos > 0.98, (n, cos)       # two 4-bit trajectories (graph vs eager kernels' rounding): bin-flip scale
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size = 128


# ------------------------------------------------------------------------------------------------ Office / DANN (N3)
@pytest.mark.parametrize("channels_last,fuse_relu,dual", [(False, False, False), (True, True, False), (True, True, True)])
def test_office_tiny_dann_two_iterations_vs_reference(dev, channels_last, fuse_relu, dual):
    """SURVEY §8f-N3 at value level: OfficeTrainStep on the tiny DANN of fixture G10 (captured from the reference's own
    dann_office model through main.py:343-456's sequence; the eager restatement reproduces it to 1e-6 on CPU,
    tests/test_oracle_torch.py) — two iterations with the per-epoch SGD re-creation (new_epoch) between them.
    Checked by value: class / domain logits, both trans losses, every site's D == the TARGET pass's D (and not the source
    pass's), alterD / gamma after ADMM_OPT.step, parameters and momentum buffers after SGD.step (momentum restarts in
    epoch 2).  Whole-network comparison is at bin-flip scale (4-bit activations flip on 1e-6 convolution differences)."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from det_init import det_init_, sample
    from alignq_amd import config
    from alignq_amd.resnet_office import DANN, Bottleneck, ResNet
    from alignq_amd.train_step import OfficeTrainStep
    g = load_golden("g10_office_tiny_dann")
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = 6
    try:
        torch.manual_seed(0)
        net = DANN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, str(g["stage"]))
        assert [n for n, _ in net.named_parameters()] == list(g["names"])
        det_init_(net)
        net = net.to(dev).train()
        # (True, True, *): every batch-norm on the folded kernels (round 3); dual: source + target pass as ONE traversal
        step = OfficeTrainStep(net, lr=float(g["lr"]), alpha=float(g["alpha"]), channels_last=channels_last,
                               fuse_relu=fuse_relu, dual=dual)
        assert step.dual == dual
        named = list(net.named_parameters())
        blocks = step.blocks
        init_state = {n: p.detach().clone() for n, p in named}
        prev = None
        for it, epoch in enumerate((1, 2)):
            rate = step.new_epoch(epoch, int(g["num_epochs"]), float(g["lr"]))
            assert abs(rate - float(g[f"rate_{it}"])) < 1e-12
            cls_s, loss, tl = step(cu(g["xs"][it], dev), cu(g["ys"][it], dev), cu(g["xt"][it], dev))
            torch.cuda.synchronize()
            # Bars: the reference's OWN response to a 1e-6 relative input perturbation (tools/office_sensitivity.py, eager
            # restatement on CPU): it0 logits 0 / D 3.0e-3 / stem weight 7.7e-4; it1 logits 0.79 / D 1.3e-2 / stem 2.8e-3
            # (4-bit bins flip and one optimiser step amplifies them).  Measured here: it0 logits <= 0.06, D <= 2.7e-3,
            # stem 6.2e-4; it1 D <= 1.1e-2 — i.e. at that floor.  What stays discriminating at WHOLE-MODEL level: both trans
            # losses (rtol 2e-4) and that D is the TARGET pass's (5-10x closer than to the source's); the first forward's logits
            # only to 0.2 (4-bit bins flip on 1e-6 convolution differences: measured 0.06).  The TIGHT per-site check of the
            # Office forward / backward is the teacher-forced Bottleneck fixture G13 (tests/test_gpu_round3.py::
            # test_teacher_forced_office_bottleneck_on_the_hip_paths: every site fed the reference's own inputs, x_q bit for bit
            # up to tie-zone flips, D / loss / gradients to 1e-5) - a wrong eps or ReLU order in one site fails there.
            if it == 0:
                np.testing.assert_allclose(npy(cls_s), g["cls_s_0"], atol=0.2)
            np.testing.assert_allclose(float(tl), float(g[f"tl_s_{it}"]) + float(g[f"tl_t_{it}"]), rtol=2e-4)
            np.testing.assert_allclose(float(loss), float(g[f"loss_{it}"]), rtol=2e-2)
            for bi, b in enumerate(blocks):
                D = npy(b.admm0.D)
                d_tgt = np.abs(D - g[f"D_{it}_{bi}"]).max()
                d_src = np.abs(D - g[f"Dsrc_{it}_{bi}"]).max()
                assert d_tgt < (6e-3, 3e-2)[it] and d_tgt < 0.4 * d_src, (it, bi, d_tgt, d_src)   # the TARGET pass's D
            for j, (n, p) in enumerate(named):
                ref = g[f"after_{it}/{j}"]
                got = npy(sample(p))
                if "alterD" in n or "gamma" in n:      # closed form of the target D: inherits D's deviation
                    np.testing.assert_allclose(got, ref, atol=(6e-3, 2e-2)[it], err_msg=n)
                else:
                    np.testing.assert_allclose(got, ref, atol=(2.5e-3, 8e-3)[it], err_msg=n)
            # the step itself, where it is not chaotic: the two heads (their inputs are the pooled features).  Update of
            # iteration it = after_it - after_(it-1): direction and size must match the reference's, which pins the
            # per-group learning rates of new_epoch (heads: rate, features: rate / 10) and the momentum restart
            # (epoch 2's buffer is the bare gradient again; carrying 0.9 * old over would double the step).
            for j, (n, p) in enumerate(named):
                if not (n.startswith("class_classifier") or n.startswith("domain_classifier")) or p.dim() != 2:
                    continue
                prev_ref = g[f"after_{it - 1}/{j}"] if it else npy(sample(init_state[n]))
                prev_got = prev[n] if it else npy(sample(init_state[n]))
                d_ref, d_got = g[f"after_{it}/{j}"] - prev_ref, npy(sample(p)) - prev_got
                cos = float((d_ref * d_got).sum() / (np.linalg.norm(d_ref) * np.linalg.norm(d_got) + 1e-30))
                ratio = float(np.linalg.norm(d_got) / (np.linalg.norm(d_ref) + 1e-30))
                assert cos > (0.99, 0.8)[it] and abs(ratio - 1.0) < (0.05, 0.3)[it], (n, it, cos, ratio)
                buf = npy(sample(step.optimizer_t.state[p]["momentum_buffer"]))
                refb = g[f"buf_{it}/{j}"]
                rb = float(np.linalg.norm(buf) / (np.linalg.norm(refb) + 1e-30))
                assert abs(rb - 1.0) < (0.05, 0.3)[it], (n, it, rb)
            prev = {n: npy(sample(p)) for n, p in named}
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100


# ------------------------------------------------------------------------------------------------ N2: integer bin storage
@pytest.mark.parametrize("formula", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 4, 6, 7, 8])
def test_packed_bins_bit_exact_and_dequant_identity(dev, formula, k):
    """the narrow integer bins (int8 while r*n <= 127, else int16; CDF tree: uint8 for k <= 8) are
    bit-exact against the oracle's bins (oq_act_quant_fwd), the dequantised value equals idx / n EXACTLY as the oracle
    divides it (bit-identical to the fused quantiser's fp32 x_q), and the packed backward equals the fp32-masked one."""
    from alignq_amd import ops
    rng = np.random.default_rng(100 * formula + k)
    x = np.concatenate([rng.standard_normal((1 << 18) + 3) * 1.7, rng.uniform(-6, 6, 1021),
                        np.array([0.0, -0.0, 30.0, -30.0, np.inf, -np.inf])]).astype(np.float32)
    n = 2 ** k - 1
    want = {(0, True): torch.int8, (0, False): torch.int16, (1, True): torch.uint8}[(formula, formula == 1 or 2.0 * n <= 127 or k == 1)]
    assert ops.bin_dtype(k, 2.0, formula) == want
    xt = cu(x, dev)
    bins, xq = ops.act_quant_pack(xt, k, 2.0, formula, want_xq=True)
    oq, ot, ob = O.act_quant_fwd(x, k, 2.0, formula)
    assert bins.dtype == want and np.array_equal(npy(bins).astype(np.int32), ob)
    assert np.array_equal(npy(xq).view(np.uint32), oq.view(np.uint32))
    deq = ops.dequant_bins(bins, k, 2.0, formula)
    # the same fp32 value everywhere; the only bit difference: round(t*n) = -0.0 for tiny negative t, which an integer
    # cannot carry (x_q = -0.0 vs dequantised +0.0, equal as numbers)
    d = npy(deq)
    assert np.array_equal(d, oq), "dequantised bins != fused quantiser's x_q"
    diff_bits = d.view(np.uint32) != oq.view(np.uint32)
    assert (oq[diff_bits] == 0).all() and np.signbit(oq[diff_bits]).all()
    if formula == 0 and k > 1:          # value == idx / n exactly (IEEE division), range as SURVEY F5
        assert np.array_equal(npy(deq), (ob.astype(np.float32) / np.float32(n)))
        assert ob.min() >= -2 * n and ob.max() <= 2 * n
    deq_r = ops.dequant_bins(bins, k, 2.0, formula, relu=True)
    assert np.array_equal(npy(deq_r), np.maximum(oq, np.float32(0)))
    # backward: mask from the bins == mask from fp32 relu(x_q)
    m = 1 << 16
    g = torch.randn(m, device=dev)
    xa = xt[:m].clone().requires_grad_(True)
    ya = ops.ActQuantReluFn.apply(xa, k, 2.0, formula)
    ya.backward(g)
    xb = xt[:m].clone().requires_grad_(True)
    yb, bb = ops.ActQuantPackedFn.apply(xb, k, 2.0, formula, True)
    yb.backward(g)
    assert np.array_equal(npy(ya), npy(yb)) and np.array_equal(npy(xa.grad), npy(xb.grad))
    assert bb.dtype == want and bb.element_size() in (1, 2)
    with pytest.raises(RuntimeError):
        ops.act_quant_pack(xt, 32, 2.0, formula)


# ------------------------------------------------------------------------------------------------ RCCL paths at world size 1
@pytest.fixture(scope="module")
def pg(dev):
    """A one-rank process group on RCCL (backend "nccl"): exercises the collective code paths on the real backend."""
    import socket
    import torch.distributed as dist
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    yield dist
    dist.destroy_process_group()


def test_global_corr_on_rccl_matches_the_fused_site(dev, pg):
    """N4 on the GPU path: dp.global_corr (all_to_all_single + all_reduce on RCCL, per-shard SYRK on the HIP kernels) at
    world size 1 equals ops.CorrFn, and a site run with config.args.global_corr gives the fused site's x_q (bit for bit),
    D, loss and dx."""
    import alignq_amd.cdf_alignment_admm as A
    from alignq_amd import _lib as L
    from alignq_amd import config, dp, ops
    torch.manual_seed(0)
    x0 = torch.randn(64, 8, 8, 8, device=dev) * 1.2
    xa = x0.clone().requires_grad_(True)
    G = dp.global_corr(xa, 0.0)
    dG = torch.randn(64, 64, device=dev)
    G.backward(dG)
    xb = x0.clone().requires_grad_(True)
    Gb = ops.CorrFn.apply(xb.view(64, -1), 0.0)
    Gb.backward(dG)
    assert np.array_equal(npy(G), npy(Gb)) and np.array_equal(npy(xa.grad), npy(xb.grad))
    gq = torch.randn_like(x0) * 0.01
    res = []
    try:
        for glob in (False, True):
            config.args.global_corr = True if glob else None
            torch.manual_seed(1)
            admm = A.ADMM(64).to(dev)
            act = A.activation_quantize_fn(8, "second", admm)
            x = x0.clone().requires_grad_(True)
            xq, loss = act(x)
            (loss + (xq * gq).sum()).backward()
            res.append((npy(xq), npy(admm.D), float(loss.detach()), npy(x.grad), npy(admm.alterD.grad)))
    finally:
        config.args.global_corr = None
    (q0, D0, l0, dx0, dA0), (q1, D1, l1, dx1, dA1) = res
    assert np.array_equal(q0, q1)
    np.testing.assert_allclose(D1, D0, atol=TOL)
    np.testing.assert_allclose(l1, l0, atol=TOL)
    np.testing.assert_allclose(dx1, dx0, atol=TOL, rtol=1e-4)
    np.testing.assert_allclose(dA1, dA0, atol=1e-7, rtol=1e-4)
    with pytest.raises(RuntimeError, match="exceeds"):
        dp.global_corr(torch.randn(1025, 64, device=dev), 0.0)
    # above 128 rows the shard SYRK is the blocked Gram (round 3): same value as the stand-alone corr
    xl = torch.randn(192, 640, device=dev)
    np.testing.assert_allclose(npy(dp.global_corr(xl, 0.0)), npy(ops.CorrFn.apply(xl, 0.0)), atol=1e-6)
    # round 4: the pair from ONE exchange of x (dp.global_site_D on ops.SiteDFn) against the two-correlation composition and
    # the oracle, in every batch regime of the site kernels (<= 32, <= 64, <= 128 rows, blocked Gram above), x_q not written
    for Bq, Fq, eps in ((28, 512, 1e-5), (48, 320, 0.0), (128, 1024, 0.0), (192, 640, 1e-5)):
        x1 = (torch.randn(Bq, Fq, device=dev) * 1.1).requires_grad_(True)
        dD = torch.randn(Bq, Bq, device=dev) * 0.1
        D1 = dp.global_site_D(x1, 4, 2.0, eps)
        D1.backward(dD)
        x2 = x1.detach().clone().requires_grad_(True)
        t2 = ops.ActQuantFn.apply(x2, 32, 2.0, L.FORMULA_ADMM)
        D2 = dp.global_corr(t2, eps) - dp.global_corr(x2, eps)
        D2.backward(dD)
        np.testing.assert_allclose(npy(D1), npy(D2), atol=TOL)
        np.testing.assert_allclose(npy(x1.grad), npy(x2.grad), atol=TOL, rtol=1e-4)
        oD = O.site_fwd(npy(x1), 4, 2.0, eps)[1]
        np.testing.assert_allclose(npy(D1), oD, atol=TOL)
        np.testing.assert_allclose(npy(x1.grad), O.site_bwd(np.zeros((Bq, Fq), np.float32), npy(dD), npy(x1), 2.0, eps), atol=TOL, rtol=1e-4)


def test_capture_after_an_eager_exact_global_phase(dev):
    """Round 4 hid two failures behind refusals; round 5:
      * capturing a step object after an eager exact-global phase crashed inside hipStreamEndCapture.  Cause: the iteration's
        autograd graph was still alive (ADMM.D is stored with its history in that mode, utils/admm.py:25; the step returned
        its loss tensors with theirs), so every parameter's gradient-accumulation node - bound to the stream the EAGER
        iteration ran on - was reused by the captured backward, and autograd's stream synchronisation pulled that stream into the
        capture.  Fixed at the source (dp.detach and capture() drop D's history, the step returns detached results) and guarded
        (train_step.retained_graph_params: a graph the caller still holds is refused with the reason, before the warm-up);
      * the exact-global mode itself stays eager-only, refused before anything touches the model, for the reason its message gives.
    The sequence runs in a child process with a hard timeout, once (tests/capture_after_detach_child.py)."""
    import socket
    import subprocess
    import sys as _sys
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "capture_after_detach_child.py")
    r = subprocess.run([_sys.executable, child, str(port)], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK ")


def test_captured_dp_step_keeps_its_bucket_across_a_short_batch(dev, pg):
    """ADVICE r2 (high).  A captured TrainStep with the data-parallel hook (world size 1 on RCCL, force=True): capture, a
    SHORT last batch (eager fallback: the hook lays out a second bucket for the [b',b'] D matrices), then a full batch again.
    The eager reduce() between the two graphs must all-reduce the buffer the graphs pack into and unpack from: checked by
    turning the collective into "multiply the reduced buffer by 2" and observing the doubled gradients in the step's result."""
    from alignq_amd import config, dp
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    from alignq_amd.train_step import TrainStep
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    torch.manual_seed(5)
    x = torch.randn(128, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (128,), device=dev)
    net = PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 8, 8, "second", 10).to(dev).train()
    step = TrainStep(net, lr=0.01, channels_last=True)
    hook = dp.attach(step, force=True)
    step.capture(x, y, warmup=2)
    assert step._graph2 is not None
    cap_bucket = hook.bucket
    step(x, y)
    step(x[:80], y[:80])                       # CIFAR's last batch: 80 of 128 (no drop_last in the reference's loaders)
    assert hook.bucket is cap_bucket and len(hook._buckets) == 2       # the fallback used its own bucket and put this one back
    seen = []
    orig = hook.reduce

    def doubling_reduce():
        seen.append(hook.bucket)
        hook.bucket.flat.mul_(2.0)             # stands in for a SUM over two identical ranks
    hook.reduce = doubling_reduce
    # a 1-D parameter (a batch-norm bias: storage order == logical order) and its offset in the flat bucket
    off, probe = 0, None
    for p_ in hook.params:
        if p_.grad is None:
            continue
        if p_.grad.dim() == 1:
            probe = p_
            break
        off += p_.numel()
    assert probe is not None
    grp = step.optimizer_t.param_groups[0]
    try:
        torch.cuda.synchronize()
        step._graph.replay()
        torch.cuda.synchronize()
        packed = cap_bucket.flat.clone()       # what graph 1 packed (this step's local gradients and D)
        p_old = probe.detach().clone()
        buf_old = step.optimizer_t.state[probe]["momentum_buffer"].clone()
        hook.reduce()
        step._graph2.replay()                  # unpack + optimiser steps
        torch.cuda.synchronize()
    finally:
        hook.reduce = orig
    assert seen == [cap_bucket]
    # graph 2 unpacked the DOUBLED buffer into the gradients SGD read: recover SGD's input gradient from its momentum update
    # (buf' = momentum * buf + (g + wd * p), utils/optimizer.py:229-245; SGD.step overwrites p.grad itself)
    buf_new = step.optimizer_t.state[probe]["momentum_buffer"]
    g_in = buf_new - grp["momentum"] * buf_old - grp["weight_decay"] * p_old
    np.testing.assert_allclose(npy(g_in), 2.0 * npy(packed[off:off + probe.numel()]), rtol=2e-3, atol=1e-6)


def test_office_step_with_bucketed_allreduce_at_world_one(dev, pg):
    """dp.attach_office(force=True): the Office step with its gradient buckets all-reduced on RCCL from autograd hooks
    (eager) and between two HIP graphs (captured); at world size 1 the mean is the identity, so both must track the plain
    step (same bars as graph-vs-eager elsewhere: MIOpen's atomics and 4-bit bin flips)."""
    from alignq_amd import config, dp
    from alignq_amd.resnet_office import DANN, Bottleneck, ResNet
    from alignq_amd.train_step import OfficeTrainStep
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = 6
    try:
        def make():
            torch.manual_seed(7)
            return DANN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1]), 8, 8, "aligned").to(dev).train()
        g = torch.Generator().manual_seed(0)
        xs = torch.randn(6, 3, 64, 64, generator=g).to(dev)
        xt = torch.randn(6, 3, 64, 64, generator=g).to(dev)
        ys = torch.randint(0, 31, (6,), generator=g).to(dev)
        m0, m1, m2 = make(), make(), make()
        s0 = OfficeTrainStep(m0, lr=0.004)
        s1 = OfficeTrainStep(m1, lr=0.004)
        h1 = dp.attach_office(s1, force=True, bucket_bytes=4 << 20)
        s2 = OfficeTrainStep(m2, lr=0.004)
        h2 = dp.attach_office(s2, force=True, bucket_bytes=4 << 20)
        for _ in range(3):
            s0(xs, ys, xt)
            s1(xs, ys, xt)
        torch.cuda.synchronize()
        assert len(h1._groups) >= 4 and h1.launched_from_hooks == 2 * len(h1._groups)      # iterations 2 and 3 overlapped
        assert sum(p.numel() for g_ in h1._groups for p in g_) == sum(p.numel() for p in m1.parameters() if p.grad is not None)
        s2.capture(xs, ys, xt, warmup=2)
        assert s2._graph2 is not None
        s2(xs, ys, xt)
        torch.cuda.synchronize()
        for (n, p0), (_, p1), (_, p2) in zip(m0.named_parameters(), m1.named_parameters(), m2.named_parameters()):
            for p in (p1, p2):
                d = np.abs(npy(p0) - npy(p))
                assert np.isfinite(d).all() and np.median(d) < 1e-3 and d.max() < 3e-2, (n, float(np.median(d)), float(d.max()))
    finally:
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100


def test_resnet50_dann_loss_trajectory_tracks_the_reference_restatement(dev):
    """`bench.py --model resnet50_dann` ended at a loss of 265 — learning rate / random init, or a bug?
    The eager restatement of the reference (pinned to it by fixture G10) run on the CPU from the same deterministic init on
    the same fixed batch gives the curves of tests/golden/g12_office_r50_trajectory.json: at the reference's default lr 0.04
    (meant for ImageNet-pretrained weights, which need the network) the loss climbs from 20 to 600 within 8 iterations, at
    0.004 it oscillates between 8 and 45.  The HIP step must follow the SAME curves (4-bit-flip-free 8-bit nets, but 8
    optimiser steps amplify rounding: 25 % per point), i.e. the blow-up is the algorithm's response to random init."""
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from det_init import det_init_
    from alignq_amd import config
    from alignq_amd.resnet_office import resnet50_dann
    from alignq_amd.train_step import OfficeTrainStep
    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "g12_office_r50_trajectory.json")))
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = 6
    try:
        g = torch.Generator().manual_seed(0)
        xs = torch.randn(6, 3, 224, 224, generator=g).to(dev)
        xt = torch.randn(6, 3, 224, 224, generator=g).to(dev)
        ys = torch.randint(0, 31, (6,), generator=g).to(dev)
        for lr in (0.04, 0.004):
            torch.manual_seed(0)
            net = det_init_(resnet50_dann(8, 8)).to(dev).train()
            step = OfficeTrainStep(net, lr=lr, alpha=0.5, channels_last=True)
            want = ref[f"lr_{lr}"]
            for it in range(6):
                _, loss, tl = step(xs, ys, xt)
                got_l, got_t = float(loss.detach()), float(tl.detach())
                assert abs(got_l - want[it][0]) <= 0.25 * want[it][0] + 0.5, (lr, it, got_l, want[it][0])
                assert abs(got_t - want[it][1]) <= 2e-3 * want[it][1] + 2e-3, (lr, it, got_t, want[it][1])
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100


def test_batch_contract_is_a_clear_python_error(dev):
    """2 <= B <= 128 is a contract of the FUSED site kernels (round 3: corr alone goes to 1024 rows, and the module
    layer composes the site from it above 128); the Python API says so instead of passing ALIGNQ_EUNSUPPORTED through."""
    from alignq_amd import ops
    for B in (1, 1025):
        with pytest.raises(RuntimeError, match="batch of 2..1024"):
            ops.CorrFn.apply(torch.randn(B, 64, device=dev), 0.0)
    for B in (1, 129):
        with pytest.raises(RuntimeError, match="batch of 2..128"):
            ops.SiteFn.apply(torch.randn(B, 64, device=dev), torch.rand(129, 129, device=dev), torch.rand(129, 129, device=dev),
                             8, 2.0, 0.0, 0.2, 0.3)


def test_teacher_forced_sites_of_the_tiny_resnet_on_the_hip_path(dev):
    """G8b: per-site teacher forcing.  The inputs the reference's own tiny PreActResNet fed to three of its
    activation sites (captured by forward hooks in model context) go through the HIP site (ops.SiteFn, and the small-batch
    kernels that B = 8 selects): x_q bins exact outside the tie zone, D / trans loss within 1e-5 of the reference — the tight
    counterpart of the whole-model G8 comparison, which can only hold at bin-flip scale."""
    from alignq_amd import ops
    g = load_golden("g8b_tiny_resnet_sites")
    k, r = int(g["k"]), float(g["act_range"])
    n = 2 ** k - 1
    for name in ("stem", "b0q1", "b2q0"):
        x = cu(g[f"{name}/x"], dev)
        A, Gm = cu(g[f"{name}/alterD"], dev), cu(g[f"{name}/gamma"], dev)
        xq, loss, D = ops.SiteFn.apply(x, A, Gm, k, r, 0.0, 0.2, 0.3)
        _, t, _ = O.act_quant_fwd(g[f"{name}/x"], k, r, O.FORMULA_ADMM)
        frac = t.astype(np.float64) * n
        tie = np.abs(frac - np.floor(frac) - 0.5) < 1e-4
        diff = np.abs(npy(xq) - g[f"{name}/xq"]) * n
        assert np.all(diff[~tie] == 0) and np.all(diff[tie] <= 1.0 + 1e-3), name
        np.testing.assert_allclose(npy(D), g[f"{name}/D"], atol=TOL, err_msg=name)
        np.testing.assert_allclose(float(loss), float(g[f"{name}/loss"]), atol=TOL, err_msg=name)
