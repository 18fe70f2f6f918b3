"""The 3x3 / padding 1 convolution of a 3-channel image (csrc/k3image_kernels.hip, include/alignq_k3image.h; ops.QConvK3ImageFn,
fused.stem_eval_into, densenet.use_hip_convs(stem=True)): bit for bit against int64 sums on operands whose every partial sum is exact
in fp32 (so the result does not depend on the accumulation order), against fp64 on dense inputs at the bar of tests/test_gpu_k3conv.py,
and as DenseNet's stem in training and in the captured evaluation.  Reference op: cdf_alignment/dense-cifar-10/model/densenet.py's
conv1 (F.conv2d(input, weight_q, None, 1, 1))."""
import ctypes

import pytest
import torch

from tests.test_gpu_k3conv import _wq, bar, count_calls

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F = torch.nn.functional
I64 = torch.int64
SENTINEL = -7.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _image(B, H, W, seed, big_everywhere):
    """i with x = i * 2^-10: |i| <= 63, and 17-bit values with live middle and low bytes in channel 0 at the pixels h % 4 == w % 4 == 1
    (any 3 x 3 window holds at most one) - or, for the filter gradient, at one such pixel per image"""
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(-63, 64, (B, H, W, 3), generator=g, dtype=I64)
    big = ((1 << 16) + (torch.randint(1, 256, (B, H, W), generator=g, dtype=I64) << 8) + torch.randint(1, 256, (B, H, W), generator=g, dtype=I64))
    big = big * (2 * torch.randint(0, 2, (B, H, W), generator=g, dtype=I64) - 1)
    at = torch.zeros(B, H, W, dtype=torch.bool)
    if big_everywhere:
        at[:, 1::4, 1::4] = True
    else:
        at[:, min(1, H - 1), min(1, W - 1)] = True
    i[..., 0] = torch.where(at, big, i[..., 0])
    return i


def _windows(i):
    """[ky][kx] -> the (B, H, W, 3) image shifted to the tap, zeros outside"""
    B, H, W, _ = i.shape
    p = F.pad(i, (0, 0, 1, 1, 1, 1))
    return [[p[:, ky:ky + H, kx:kx + W] for kx in range(3)] for ky in range(3)]


def _conv_i64(i, b):
    win = _windows(i)
    return sum(torch.einsum("bhwc,oc->bhwo", win[ky][kx], b[:, ky, kx]) for ky in range(3) for kx in range(3))


def _wgrad_i64(i, j):
    win = _windows(i)
    return torch.stack([torch.stack([torch.einsum("bhwo,bhwc->oc", j, win[ky][kx]) for kx in range(3)], 1) for ky in range(3)], 1)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("w_bit", [8, 2])
@pytest.mark.parametrize("B,H,W,cout,ldy", [(1, 1, 1, 4, 4), (2, 9, 11, 24, 24), (2, 8, 8, 32, 40), (1, 17, 5, 68, 68)])
def test_forward_is_the_quotient_of_the_integer_sum(dev, B, H, W, cout, ldy, w_bit):
    from alignq_amd import _lib as L
    lib, n = L.load(), 2 ** w_bit - 1
    lim = min(n, 31)
    i = _image(B, H, W, 7 * H + cout, True)
    b = torch.randint(-lim, lim + 1, (cout, 3, 3, 3), generator=torch.Generator().manual_seed(cout + w_bit), dtype=I64)   # [co][ky][kx][ci]
    assert int(_conv_i64(i.abs(), b.abs()).max()) < 2 ** 24          # every partial sum is exact in fp32
    ref = (_conv_i64(i, b).double() * 2.0 ** -10).float() / torch.tensor(float(n), dtype=torch.float32)
    x = (i.double() * 2.0 ** -10).float().to(dev)
    wb = b.to(torch.bfloat16).view(torch.int16).to(dev)
    outs = []
    for _ in range(2):
        y = torch.full((B, H, W, ldy), SENTINEL, device=dev)
        L.check(lib.alignq_k3image_fwd(L.ptr(x), L.ptr(wb), L.ptr(y), B, H, W, cout, ldy, w_bit, L.stream_ptr()), "alignq_k3image_fwd")
        outs.append(y.cpu())
    assert torch.equal(_bits(outs[0][..., :cout]), _bits(ref)), float((outs[0][..., :cout] - ref).abs().max())
    assert bool((outs[0][..., cout:] == SENTINEL).all()), "a channel beyond COUT was written"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two launches on the same inputs differ"


@pytest.mark.parametrize("B,H,W,cout", [(1, 4, 8, 4), (3, 9, 11, 24), (2, 16, 16, 68)])
def test_filter_gradient_is_the_integer_sum(dev, B, H, W, cout):
    from alignq_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(H + cout)
    i = _image(B, H, W, 3 * H + cout, False)
    pix = torch.arange(B * H * W).reshape(B, H, W, 1) + torch.arange(cout)
    j = torch.randint(-15, 16, (B, H, W, cout), generator=g, dtype=I64) * (pix % 3 == 0)          # dy = j * 2^-6
    assert int(_wgrad_i64(i.abs(), j.abs()).max()) < 2 ** 24
    ref = (_wgrad_i64(i, j).double() * 2.0 ** -16).float().reshape(-1)
    x, dy = (i.double() * 2.0 ** -10).float().to(dev), (j.double() * 2.0 ** -6).float().to(dev)
    n_elem, nws = cout * 27, lib.alignq_k3image_wgrad_ws_bytes(B, H, W, cout)
    outs = []
    for deferred in (False, False, True):
        ws = torch.full((nws // 4,), float("nan"), device=dev)
        dw = torch.full((n_elem,), float("nan"), device=dev)
        ns = ctypes.c_int(0)
        L.check(lib.alignq_k3image_wgrad(L.ptr(x), L.ptr(dy), None if deferred else L.ptr(dw), L.ptr(ws), B, H, W, cout,
                                         ctypes.byref(ns) if deferred else None, L.stream_ptr()), "alignq_k3image_wgrad")
        if deferred:
            assert ns.value * n_elem * 4 == nws
            L.check(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws]), L.ptr_array([dw]), (ctypes.c_int * 1)(ns.value),
                                                          (ctypes.c_int * 1)(n_elem), L.stream_ptr()), "alignq_conv3x3_wgrad_reduce_multi")
        assert bool(torch.isfinite(ws).all()), "a slab element was not written"
        outs.append(dw.cpu())
    assert torch.equal(_bits(outs[0]), _bits(ref)), float((outs[0] - ref).abs().max())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two launches on the same inputs differ"
    assert torch.equal(_bits(outs[0]), _bits(outs[2])), "the deferred reduction differs from the stand-alone one"


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("B,H,W,cout", [(2, 9, 11, 24), (4, 32, 32, 32)])
def test_function_matches_fp64(dev, B, H, W, cout, k):
    from alignq_amd import ops
    seed = cout + H + k
    wq = _wq(cout, 3, k, dev, seed).requires_grad_(True)
    x = (torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed + 1)) * 1.3).to(dev).contiguous(memory_format=CL)
    gy = (torch.randn(B, cout, H, W, generator=torch.Generator().manual_seed(seed + 2)) * 1e-3).to(dev).contiguous(memory_format=CL)
    assert ops.qconv_k3_image_supported(x, wq, (1, 1), (1, 1), (1, 1), 1, None, k)
    assert not ops.qconv_k3_image_supported(x.clone().requires_grad_(True), wq, (1, 1), (1, 1), (1, 1), 1, None, k)
    runs = []
    for _ in range(2):
        wq.grad = None
        y = ops.QConvK3ImageFn.apply(x, wq, k)
        y.backward(gy)
        runs.append((y.detach(), wq.grad))
    y, dw = runs[0]
    assert y.is_contiguous(memory_format=CL) and dw.is_contiguous(memory_format=CL) and dw.shape == wq.shape
    xd, wd = x.double(), wq.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, None, 1, 1)
    yd.backward(gy.double())
    y32 = F.conv2d(x, wq.detach(), None, 1, 1)
    dw32 = torch.ops.aten.convolution_backward(gy, x, wq.detach(), None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))[1]
    bar(y, yd.detach(), y32, "3->%d %dx%d k=%d fwd" % (cout, H, W, k))
    bar(dw, wd.grad, dw32, "3->%d %dx%d k=%d wgrad" % (cout, H, W, k))
    assert torch.equal(_bits(y), _bits(runs[1][0])) and torch.equal(_bits(dw), _bits(runs[1][1])), "a second launch differs"


# ------------------------------------------------------------------------------------------------ in the network, depth 10
def _net(dev, stem, dense_eval=False):
    from alignq_amd import densenet as D
    torch.manual_seed(5)
    return D.use_hip_convs(D.DenseNet(4, 4, "no_align", depth=10, compressionRate=1).to(dev), dense_eval=dense_eval, stem=stem)


def test_stem_in_training(dev, monkeypatch):
    """conv1 with and without the flag, and - the fp64 statement - the same filter convolved in fp64 behind the same quantiser"""
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(dev).contiguous(memory_format=CL)
    gy = torch.randn(2, 24, 32, 32, generator=torch.Generator().manual_seed(7)).to(dev).contiguous(memory_format=CL) * 1e-3
    calls = count_calls(monkeypatch, "alignq_k3image_fwd")
    off, on, ref = _net(dev, False), _net(dev, True), _net(dev, False)
    y_off = off.conv1(x)
    y_off.backward(gy)
    assert calls["alignq_k3image_fwd"] == 0
    y_on = on.conv1(x)
    y_on.backward(gy)
    assert calls["alignq_k3image_fwd"] == 1
    yd = F.conv2d(x.double(), ref.conv1.quantize_fn(ref.conv1.weight).double(), None, 1, 1)
    yd.backward(gy.double())
    bar(y_on.detach(), yd.detach(), y_off.detach(), "conv1 output")
    bar(on.conv1.weight.grad, ref.conv1.weight.grad.double(), off.conv1.weight.grad, "conv1.weight.grad")


def test_eval_step_writes_the_stem_into_the_block_buffer(dev, monkeypatch):
    from alignq_amd import fused, ops
    from alignq_amd.eval_step import EvalStep
    g = torch.Generator().manual_seed(8)
    x, t = torch.randn(2, 3, 32, 32, generator=g).to(dev), torch.randint(0, 10, (2,), generator=g).to(dev)
    with EvalStep(_net(dev, False, dense_eval=True), channels_last=True, qconv=True) as ev:
        flag_off = ev(x, t).clone()

    def by_copy(conv, xx, buf):          # the twin: the first block's prefix filled with QConvK3ImageFn's output by copy_
        rec = conv.quantize_fn.parked
        buf[:, :conv.out_channels].copy_(ops.QConvK3ImageFn.apply(xx, rec.q, conv.quantize_fn.w_bit, rec.bins))
        return buf

    calls = count_calls(monkeypatch, "alignq_k3image_fwd")
    ev = EvalStep(_net(dev, True, dense_eval=True), channels_last=True, qconv=True)
    with ev:
        eager = ev(x, t).clone()
        assert calls["alignq_k3image_fwd"] == 1
        with monkeypatch.context() as mp:
            mp.setattr(fused, "stem_eval_into", by_copy)
            twin = ev(x, t).clone()
        ev.capture(x, t, warmup=1)
        replays = [ev(x, t).clone() for _ in range(3)]
    assert torch.isfinite(eager).all() and tuple(eager.shape) == (2, 10)
    assert torch.equal(_bits(eager), _bits(twin)), float((eager - twin).abs().max())
    assert all(torch.equal(_bits(r), _bits(eager)) for r in replays), "replay != eager"
    bar(eager, flag_off.double(), flag_off, "logits against the flag-off EvalStep")
