"""Conv2d_Q's 3x3 / stride 1 / padding 1 convolutions at channel counts that are multiples of 4 (csrc/k3conv_kernels.hip,
ops.QConvK3Fn) on real fp32 data: against an fp64 convolution of the same inputs at the bar of tests/test_gpu_qconv.py (restated as
`_bar` in tests/test_gpu_pointwise.py), and the backward's use of needs_input_grad.  Reference op:
cdf_alignment/dense-cifar-10/model/quantization.py (F.conv2d(input, weight_q, ...)), shapes of model/densenet.py:17-41."""
import pytest
import torch

from tests.k3conv_exact_oracle import SHAPES as CHANNELS

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F = torch.nn.functional
# (CIN, COUT, B, H): the channel pairs of tests/k3conv_exact_oracle.py at 3 x 5 x 5, and three real DenseNet-40 layers at B = 3
SHAPES = [(ci, co, 3, 5) for ci, co in CHANNELS] + [(24, 12, 3, 32), (168, 12, 3, 16), (444, 12, 3, 8)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def count_calls(monkeypatch, *names):
    from alignq_amd import _lib as L
    lib = L.load()
    calls = {n: 0 for n in names}
    for n in names:
        def wrapper(*a, _orig=getattr(lib, n), _n=n):
            calls[_n] += 1
            return _orig(*a)
        monkeypatch.setattr(lib, n, wrapper)
    return calls


def _wq(cout, cin, k, dev, seed):
    g = torch.Generator().manual_seed(seed)
    n = 2 ** k - 1
    w = torch.round(torch.tanh(torch.randn(cout, cin, 3, 3, generator=g)) * n) / n
    return w.to(dev).contiguous(memory_format=CL)


def bar(got, ref64, torch32, what):
    """tests/test_gpu_qconv.py::_check's bar: no further from the fp64 result than torch's own fp32 convolution on the same inputs, or
    2e-6 of the largest fp64 magnitude"""
    floor = 2e-6 * float(ref64.abs().max())
    err, err32 = float((got.double() - ref64).abs().max()), float((torch32.double() - ref64).abs().max())
    print("%s: max err %.3e, torch fp32 %.3e, floor %.3e" % (what, err, err32, floor))
    assert err <= max(err32, floor), (what, err, err32, floor)


def check_layer(x, wq, gy, y, dx, dw, what):
    """y, dx, dw of one 3x3 layer against fp64 on its own inputs"""
    xd, wd = x.detach().double().requires_grad_(True), wq.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, None, 1, 1)
    yd.backward(gy.double())
    y32 = F.conv2d(x.detach(), wq.detach(), None, 1, 1)
    dx32, dw32 = torch.ops.aten.convolution_backward(gy, x.detach(), wq.detach(), None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                     (True, True, False))[:2]
    bar(y.detach(), yd.detach(), y32, what + " fwd")
    bar(dx, xd.grad, dx32, what + " dgrad")
    bar(dw, wd.grad, dw32, what + " wgrad")


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("cin,cout,B,H", SHAPES)
def test_qconv_k3_matches_fp64(dev, cin, cout, B, H, k):
    from alignq_amd import ops
    seed = cin + 3 * cout + H + k
    wq = _wq(cout, cin, k, dev, seed).requires_grad_(True)
    x = (torch.randn(B, cin, H, H, generator=torch.Generator().manual_seed(seed + 1)) * 1.3).to(dev).contiguous(memory_format=CL)
    x.requires_grad_(True)
    assert ops.qconv_k3_supported(x, wq, (1, 1), (1, 1), (1, 1), 1, None, k)
    y = ops.QConvK3Fn.apply(x, wq, k)
    assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (B, cout, H, H)
    gy = (torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 2)) * 1e-3).to(dev).contiguous(memory_format=CL)
    y.backward(gy)
    assert wq.grad.is_contiguous(memory_format=CL) and x.grad.is_contiguous(memory_format=CL)
    check_layer(x, wq, gy, y, x.grad, wq.grad, "%d->%d H=%d k=%d" % (cin, cout, H, k))


def test_backward_honours_needs_input_grad(dev, monkeypatch):
    from alignq_amd import ops
    calls = count_calls(monkeypatch, "alignq_k3conv_fwd", "alignq_k3conv_dgrad", "alignq_k3conv_wgrad")
    wq = _wq(12, 24, 4, dev, 1)
    x = torch.randn(2, 24, 3, 3, device=dev).contiguous(memory_format=CL)
    gy = torch.randn(2, 12, 3, 3, device=dev)                                  # not channels-last: made so by the backward
    ops.QConvK3Fn.apply(x.clone().requires_grad_(True), wq, 4).backward(gy)
    assert calls == {"alignq_k3conv_fwd": 1, "alignq_k3conv_dgrad": 1, "alignq_k3conv_wgrad": 0}
    ops.QConvK3Fn.apply(x, wq.clone().requires_grad_(True), 4).backward(gy)
    assert calls == {"alignq_k3conv_fwd": 2, "alignq_k3conv_dgrad": 1, "alignq_k3conv_wgrad": 1}


def test_filter_gradient_is_deferred_inside_a_pending_list(dev):
    """inside fused.DeferredWgrads the slabs are reduced by the one launch at the end: the same bits as the stand-alone reduction"""
    from alignq_amd import fused, ops
    wq = _wq(12, 36, 4, dev, 2)
    x = torch.randn(3, 36, 9, 9, generator=torch.Generator().manual_seed(3)).to(dev).contiguous(memory_format=CL)
    gy = torch.randn(3, 12, 9, 9, generator=torch.Generator().manual_seed(4)).to(dev).contiguous(memory_format=CL)
    w1 = wq.clone().requires_grad_(True)
    ops.QConvK3Fn.apply(x, w1, 4).backward(gy)
    w2 = wq.clone().requires_grad_(True)
    with fused.DeferredWgrads() as pending:
        ops.QConvK3Fn.apply(x, w2, 4).backward(gy)
        assert [(i[2], i[3]) for i in pending.items] == [(9, 12 * 9 * 36)]          # 3 x 3 x 2 = 18 steps in nine slabs
        dw = pending.items[0][1]          # the tensor the node returned (its consumer flushes before it reads: fused.DeferredWgrads)
        pending.flush()
    torch.cuda.synchronize()
    assert dw.shape == wq.shape and torch.equal(w1.grad.view(torch.int32), dw.view(torch.int32))
