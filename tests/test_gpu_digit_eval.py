"""The digit DANN's evaluation pass (csrc/digit_eval_kernels.hip, include/alignq_digit.h): conv 5x5 + bias -> eval-mode BN -> act_q ->
ReLU -> MaxPool2d(2) as one launch, bit for bit against the three launches it replaces (their arithmetic is fixed and the kernel states
the same one: zero tolerance is derived), against float64 at k = 32, and through EvalStep against the composition and fixture G24."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.golden.digit_init import digit_init_
from tests.test_gpu_k3conv import bar, count_calls

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F = torch.nn.functional
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.5          # (no output is negative)

# (cin, cout): one chunk with a zero tail; two chunks with a tail and an N tail; the DANN's body layer; N32; N64; the image form twice
CHANNELS = [(4, 4), (36, 20), (32, 48), (8, 32), (8, 64), (3, 32), (3, 20)]
# a single window; 9 x 8 output (odd row dropped, partial tile); 16 x 17 output (a third tile column whose only window is dropped)
SHAPES = [(1, 6, 6), (2, 13, 12), (3, 20, 21)]


def _cases():
    """pruned cross-product: every (channels, shape) pair; k, formula, w_bit, bias and layout cycle; x_channels = 1 on flat image cases"""
    out = []
    for i, (cin, cout) in enumerate(CHANNELS):
        for j, shape in enumerate(SHAPES):
            n = i + j
            flat = bool((i + (j + 1) // 2) % 2)
            out.append((cin, cout) + shape + ((2, 4, 32)[n % 3], n % 2, (2, 8)[(n // 2) % 2], (i + j // 2) % 2 == 0, flat,
                                              1 if cin == 3 and flat else cin))
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(cin, cout, B, H, W, w_bit, with_bias, xc, dev):
    g = torch.Generator().manual_seed(cin + 3 * cout + 7 * H + W + w_bit)
    n = 2 ** w_bit - 1
    wq = (torch.round(torch.tanh(torch.randn(cout, cin, 5, 5, generator=g)) * n) / n).to(dev).contiguous(memory_format=CL)
    x = (torch.randn(B, xc, H, W, generator=g) * 1.3).to(dev).contiguous(memory_format=CL)
    bias = torch.randn(cout, generator=g).to(dev) if with_bias else None
    # gamma of both signs, running_var over two decades
    sign = 1.0 - 2.0 * (torch.arange(cout) % 3 == 1)
    vecs = [v.to(dev) for v in ((torch.rand(cout, generator=g) + 0.3) * sign, torch.randn(cout, generator=g) * 0.5,
                                torch.randn(cout, generator=g), 10.0 ** (torch.rand(cout, generator=g) * 2 - 1) * (cin * 25 / 3))]
    return x, wq, bias, vecs


def _fused(x, wq, bias, vecs, k, formula, w_bit, flat, cin):
    """alignq_k5conv_site_pool_eval_fwd into a sentinel-guarded buffer; returns the (B, cout, PH, PW) result"""
    from alignq_amd import _lib as L
    from alignq_amd import ops
    B, xc, H, W = x.shape
    cout, PH, PW = wq.shape[0], (H - 4) // 2, (W - 4) // 2
    n, guard = B * PH * PW * cout, 64
    buf = torch.full((n + 2 * guard,), SENTINEL, device=x.device)
    y = buf[guard:guard + n]
    site = L.DenseSite(*(L.ptr(v) for v in vecs), 1e-5, k, L.CLAMP_RELU)
    bins = ops.pack_filter_bins([wq], w_bit)[0]
    rc = L.load().alignq_k5conv_site_pool_eval_fwd(L.ptr(x), xc, L.ptr(bins[0]), L.ptr(bias), ctypes.byref(site), L.ptr(y),
                                                   L.DIGIT_OUT_FLAT_CHW if flat else L.DIGIT_OUT_NHWC, B, H, W, cin, cout, w_bit, 2.0,
                                                   formula, L.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (buf[:guard] == SENTINEL).all() and (buf[guard + n:] == SENTINEL).all() and (y >= 0).all()
    return y.view(B, cout, PH, PW) if flat else y.view(B, PH, PW, cout).permute(0, 3, 1, 2)


def _three_launches(x, wq, bias, vecs, k, formula, w_bit):
    from alignq_amd import _lib as L
    from alignq_amd import ops
    z = ops.QConvK5Fn.apply(x, wq, bias, w_bit)
    s = torch.empty_like(z, memory_format=CL)
    site = L.EvalSite(L.ptr(z), *(L.ptr(v) for v in vecs), 1e-5, k, L.CLAMP_RELU)
    B, C, OH, OW = z.shape
    assert L.load().alignq_site_eval_fwd(ctypes.byref(site), B * OH * OW, C, 2.0, formula, None, L.ptr(s), L.stream_ptr()) == 0
    return F.max_pool2d(s, 2)


@pytest.mark.parametrize("cin,cout,B,H,W,k,formula,w_bit,with_bias,flat,xc", _cases())
def test_one_launch_gives_the_bits_of_the_three_it_replaces(dev, cin, cout, B, H, W, k, formula, w_bit, with_bias, flat, xc):
    x, wq, bias, vecs = _inputs(cin, cout, B, H, W, w_bit, with_bias, xc, dev)
    got = _fused(x, wq, bias, vecs, k, formula, w_bit, flat, cin)
    x3 = x.expand(B, cin, H, W).contiguous(memory_format=CL)
    want = _three_launches(x3, wq, bias, vecs, k, formula, w_bit)
    assert got.shape == want.shape and want.numel() > 0 and (want > 0).any()
    assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    again = _fused(x, wq, bias, vecs, k, formula, w_bit, flat, cin)
    assert torch.equal(got.contiguous().view(torch.int32), again.contiguous().view(torch.int32))


@pytest.mark.parametrize("cin,cout,B,H,W", [(32, 48, 2, 12, 12), (3, 32, 2, 28, 28)])
def test_without_a_quantiser_it_is_as_close_to_float64_as_torch(dev, cin, cout, B, H, W):
    x, wq, bias, vecs = _inputs(cin, cout, B, H, W, 8, True, cin, dev)
    got = _fused(x, wq, bias, vecs, 32, 0, 8, False, cin)

    def compose(x, wq, bias, vecs):
        z = F.batch_norm(F.conv2d(x, wq, bias), vecs[2], vecs[3], vecs[0], vecs[1], False, 0.0, 1e-5)
        return F.max_pool2d(F.relu(z), 2)
    ref64 = compose(x.double(), wq.double(), bias.double(), [v.double() for v in vecs])
    bar(got, ref64, compose(x, wq, bias, vecs), "site+pool %s" % ((cin, cout, B, H, W),))


# ------------------------------------------------------------------------------------------------------------------ EvalStep
def _model(dev, wbit=4, abit=4, fused_eval=True):
    from alignq_amd import digit
    net = digit_init_(digit.MNISTmodel_quant("org", wbit, abit)).to(dev)
    with torch.no_grad():          # running statistics that are not the defaults
        g = torch.Generator().manual_seed(5)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return digit.use_hip_convs(net, eval_fused=fused_eval)


def test_eval_step_on_the_digit_model(dev, monkeypatch):
    from alignq_amd import export, fused, paths
    from alignq_amd.eval_step import EvalStep
    net = _model(dev)
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(4, 1, 28, 28, generator=g).to(dev), torch.randint(0, 10, (4,), generator=g).to(dev)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    flags = lambda: [{k: m.__dict__[k] for k in paths.FLAGS + ("training",) if k in m.__dict__} for m in net.modules()]          # noqa: E731
    before = flags()
    calls = count_calls(monkeypatch, "alignq_k5conv_site_pool_eval_fwd", "alignq_k5conv_fwd")
    with EvalStep(net) as ev:
        assert not ev._office
        logits = ev(x, y).clone()
        assert calls == {"alignq_k5conv_site_pool_eval_fwd": 2, "alignq_k5conv_fwd": 0}
        res = ev.result()
        # the composition written out: module convolution, folded site, pool, reshape, classifier
        with torch.no_grad(), fused.eval_scope():
            h = x.expand(4, 3, 28, 28).contiguous(memory_format=CL)
            f = net.feature
            for i in (0, 5):
                h = F.max_pool2d(fused.site_eval_any(f[i + 1], f[i + 2], f[i](h), fused.CLAMP_RELU), 2)
            want = net.classifier(h.reshape(-1, 768))
        assert calls["alignq_k5conv_fwd"] == 2 and torch.equal(logits.view(torch.int32), want.view(torch.int32))
        # CE / top-1 / top-5 in NumPy on the logits
        lg, t = logits.double().cpu().numpy(), y.cpu().numpy()
        lse = np.log(np.exp(lg - lg.max(1, keepdims=True)).sum(1)) + lg.max(1)
        rank = (lg > lg[np.arange(4), t][:, None]).sum(1)
        assert abs(res[0] - float((lse - lg[np.arange(4), t]).mean())) <= 1e-6 * max(1.0, abs(res[0]))
        assert res[1:] == (100.0 * (rank < 1).mean(), 100.0 * (rank < 5).mean(), 4)
        # graph replay against eager, several replays
        ev.capture(x, y)
        for _ in range(3):
            assert torch.equal(ev(x, y).view(torch.int32), logits.view(torch.int32))
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    assert flags() == before and net.training and net.fuse_digit_eval
    # packed weights give the same logits
    pk = export.pack_model(net)
    skeleton = _model(dev)
    pk.apply(skeleton)
    with EvalStep(skeleton, weights=pk) as ev2:
        assert torch.equal(ev2(x, y).view(torch.int32), logits.view(torch.int32))
    # flag off: the step runs and makes no fused call
    calls["alignq_k5conv_site_pool_eval_fwd"] = 0
    with EvalStep(_model(dev, fused_eval=False)) as ev3:
        off = ev3(x, y)
    assert calls["alignq_k5conv_site_pool_eval_fwd"] == 0 and torch.isfinite(off).all()


def test_eval_step_against_the_reference(dev):
    """G24: max |EvalStep logits - class64| <= 2 * max(e_ref, e_off): two fp32 evaluations in different operation orders each lie within
    one such error of float64.  Measured on the MI355X: see NOTES.md, "Digit DANN evaluation"."""
    from alignq_amd import digit
    from alignq_amd.eval_step import EvalStep
    g24 = np.load(os.path.join(HERE, "golden", "g24_digit_eval.npz"))
    x, c64 = torch.from_numpy(g24["x"]).to(dev), g24["class64"]
    y = torch.zeros(4, dtype=torch.int64, device=dev)
    net = digit.use_hip_convs(digit_init_(digit.MNISTmodel_quant(str(g24["stage"]), 8, 32)).to(dev), eval_fused=True)
    with EvalStep(net) as ev:
        got = ev(x, y).double().cpu().numpy()
    net_off = digit.use_hip_convs(digit_init_(digit.MNISTmodel_quant(str(g24["stage"]), 8, 32)).to(dev)).eval()
    with torch.no_grad():
        off = net_off(x, 0.0)[0].double().cpu().numpy()
    err, e_off, e_ref = float(np.abs(got - c64).max()), float(np.abs(off - c64).max()), float(g24["e_ref"])
    print(f"G24: max |EvalStep - class64| {err:.3e}, e_off {e_off:.3e}, e_ref {e_ref:.3e}")
    assert err <= 2 * max(e_ref, e_off)
