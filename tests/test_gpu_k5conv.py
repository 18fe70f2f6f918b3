"""Conv2d_Q's 5x5 / stride 1 / padding 0 convolutions with a bias (csrc/k5conv_kernels.hip, ops.QConvK5Fn) on real fp32 data: against an
fp64 convolution of the same inputs at the bar of tests/test_gpu_k3conv.py, in both forms (body: channel counts that are multiples of
4; image: 3 input channels folded with the taps), and the backward's use of needs_input_grad and of fused.DeferredWgrads.  Reference
op: cdf_alignment/dann_digit/model/quantization.py (F.conv2d(input, weight_q, self.bias, ...)), shapes of model/dann.py:143-150."""
import pytest
import torch

from tests.test_gpu_k3conv import bar, count_calls

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F = torch.nn.functional
# body form: one chunk with a zero tail, an exact chunk, two chunks with a tail, every tile width in both directions
CHANNELS = [(4, 4), (32, 48), (36, 32), (32, 64), (64, 12)]
# one output pixel; exactly one output tile with B > 1; one pixel beyond a tile one way and below it the other
GRIDS = [(1, 5, 5), (3, 12, 12), (2, 13, 7)]
IMAGE_GRIDS = [(1, 5, 5), (3, 12, 12), (2, 28, 28)]
BITS = [(4, True), (4, False), (8, True), (8, False)]          # (w_bit, with a bias)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(cin, cout, B, H, W, k, with_bias, dev):
    g = torch.Generator().manual_seed(cin + 3 * cout + 7 * H + W + k)
    n = 2 ** k - 1
    wq = (torch.round(torch.tanh(torch.randn(cout, cin, 5, 5, generator=g)) * n) / n).to(dev).contiguous(memory_format=CL)
    x = (torch.randn(B, cin, H, W, generator=g) * 1.3).to(dev).contiguous(memory_format=CL)
    bias = torch.randn(cout, generator=g).to(dev) if with_bias else None
    gy = (torch.randn(B, cout, H - 4, W - 4, generator=g) * 1e-3).to(dev).contiguous(memory_format=CL)
    return x, wq, bias, gy


def _check(x, wq, bias, gy, k, want_dx):
    """QConvK5Fn's y, dw (and dx) against fp64 on the same inputs"""
    from alignq_amd import ops
    x = x.clone().requires_grad_(want_dx)
    wq = wq.clone().requires_grad_(True)
    assert ops.qconv_k5_supported(x, wq, (1, 1), (0, 0), (1, 1), 1, bias, k)
    y = ops.QConvK5Fn.apply(x, wq, bias, k)
    assert y.is_contiguous(memory_format=CL) and y.shape == gy.shape
    y.backward(gy)
    xd, wd = x.detach().double().requires_grad_(want_dx), wq.detach().double().requires_grad_(True)
    F.conv2d(xd, wd, None if bias is None else bias.double()).backward(gy.double())
    y64 = F.conv2d(xd.detach(), wd.detach(), None if bias is None else bias.double())
    y32 = F.conv2d(x.detach(), wq.detach(), bias)
    dx32, dw32 = torch.ops.aten.convolution_backward(gy, x.detach(), wq.detach(), None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
                                                     (want_dx, True, False))[:2]
    what = "%s k=%d" % (tuple(x.shape) + tuple(wq.shape[:1]), k)
    bar(y.detach(), y64, y32, what + " fwd")
    bar(wq.grad, wd.grad, dw32, what + " wgrad")
    assert wq.grad.is_contiguous(memory_format=CL)
    if want_dx:
        assert x.grad.shape == x.shape and x.grad.is_contiguous(memory_format=CL)
        bar(x.grad, xd.grad, dx32, what + " dgrad")


@pytest.mark.parametrize("k,with_bias", BITS)
@pytest.mark.parametrize("B,H,W", GRIDS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_body_form_matches_fp64(dev, cin, cout, B, H, W, k, with_bias):
    _check(*_inputs(cin, cout, B, H, W, k, with_bias, dev), k, True)


@pytest.mark.parametrize("k,with_bias", BITS)
@pytest.mark.parametrize("B,H,W", IMAGE_GRIDS)
@pytest.mark.parametrize("cout", [4, 32])
def test_image_form_matches_fp64(dev, cout, B, H, W, k, with_bias):
    _check(*_inputs(3, cout, B, H, W, k, with_bias, dev), k, False)


@pytest.mark.parametrize("cin,cout,B,H,W", [
    (3, 128, 3, 12, 12),          # image form: the 64-wide forward tile, two channel tiles each way
    (4, 4, 33, 68, 68),           # more spatial tiles than the grid holds (33 x 64 and 33 x 81 > 2048); outputs stored write-through
])
def test_wide_and_beyond_the_grid_cap(dev, cin, cout, B, H, W):
    _check(*_inputs(cin, cout, B, H, W, 4, True, dev), 4, cin != 3)


def test_image_form_is_refused_for_an_input_that_needs_a_gradient(dev):
    from alignq_amd import ops
    x, wq, bias, _ = _inputs(3, 32, 2, 12, 12, 4, True, dev)
    args = (wq, (1, 1), (0, 0), (1, 1), 1, bias, 4)
    assert ops.qconv_k5_supported(x, *args) and not ops.qconv_k5_supported(x.clone().requires_grad_(True), *args)
    assert not ops.qconv_k5_supported(x, wq, (1, 1), (0, 0), (1, 1), 1, bias.double(), 4)


def test_backward_honours_needs_input_grad(dev, monkeypatch):
    from alignq_amd import ops
    calls = count_calls(monkeypatch, "alignq_k5conv_fwd", "alignq_k5conv_dgrad", "alignq_k5conv_wgrad")
    x, wq, bias, gy = _inputs(32, 48, 2, 6, 6, 4, True, dev)
    gy = gy.contiguous()                                                       # not channels-last: made so by the backward
    ops.QConvK5Fn.apply(x.clone().requires_grad_(True), wq, bias, 4).backward(gy)
    assert calls == {"alignq_k5conv_fwd": 1, "alignq_k5conv_dgrad": 1, "alignq_k5conv_wgrad": 0}
    b = bias.clone().requires_grad_(True)
    ops.QConvK5Fn.apply(x, wq.clone().requires_grad_(True), b, 4).backward(gy)
    assert calls == {"alignq_k5conv_fwd": 2, "alignq_k5conv_dgrad": 1, "alignq_k5conv_wgrad": 1}
    assert torch.allclose(b.grad, gy.sum((0, 2, 3)), rtol=1e-6, atol=1e-9)


def test_filter_gradient_is_deferred_inside_a_pending_list(dev):
    """inside fused.DeferredWgrads the slabs are reduced by the one launch at the end: the same bits as the stand-alone reduction"""
    from alignq_amd import fused, ops
    x, wq, bias, gy = _inputs(36, 32, 3, 12, 12, 4, True, dev)
    w1 = wq.clone().requires_grad_(True)
    ops.QConvK5Fn.apply(x, w1, bias, 4).backward(gy)
    w2 = wq.clone().requires_grad_(True)
    with fused.DeferredWgrads() as pending:
        ops.QConvK5Fn.apply(x, w2, bias, 4).backward(gy)
        assert [(i[2], i[3]) for i in pending.items] == [(3, 32 * 25 * 36)]          # 3 x 2 x 1 = 6 steps in three slabs
        dw = pending.items[0][1]
        pending.flush()
    torch.cuda.synchronize()
    assert dw.shape == wq.shape and torch.equal(w1.grad.view(torch.int32), dw.view(torch.int32))


@pytest.mark.parametrize("cin", [3, 36])
def test_two_launches_give_the_same_bits(dev, cin):
    """forward, filter gradient and (body form) data gradient, launched twice on the same inputs"""
    from alignq_amd import ops
    x, wq, bias, gy = _inputs(cin, 48, 3, 13, 12, 4, True, dev)
    runs = []
    for _ in range(2):
        xr, wr = x.clone().requires_grad_(cin != 3), wq.clone().requires_grad_(True)
        y = ops.QConvK5Fn.apply(xr, wr, bias, 4)
        y.backward(gy)
        runs.append([y.detach(), wr.grad] + ([xr.grad] if cin != 3 else []))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
