"""Conv2d_Q's pointwise convolutions at channel counts that are multiples of 8 (csrc/pointwise_kernels.hip, ops.QConvPwFn) on real
fp32 data: against an fp64 convolution of the same inputs at the bar of tests/test_gpu_qconv.py, inside a 4W/4A MobileNet-V2
forward + backward with mobilenet.use_hip_convs(model, pointwise=True), default off, and inside eval_step.EvalStep on fixture G20
(eager, captured, from packed weights).  Reference op: cdf_alignment/mobilenet-v2-svhn/model/quantization.py (F.conv2d(input,
weight_q, ...)), shapes of model/mobilenetV2.py:25-60."""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.golden.mobilenet_init import REDUCED_CFG, mobilenet_init_
from tests.test_gpu_mobile_eval import bare_eval, reduced_net

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F = torch.nn.functional
PW_FWD, GEMM_FWD, PACK = "alignq_pwconv_fwd", "alignq_qconv_fwd", "alignq_qconv_pack_weights"
# (CIN, COUT, B, H): the shapes of tests/pointwise_exact_oracle.py at 75 pixels, and three real MobileNet-V2 layers at B = 3
SHAPES = [(ci, co, 3, 5) for ci, co in [(8, 8), (16, 96), (96, 24), (24, 144), (144, 32), (40, 200), (160, 320), (2048, 8), (8, 2048)]]
SHAPES += [(16, 96, 3, 16), (144, 24, 3, 8), (576, 160, 3, 4)]
# REDUCED_CFG: the 1x1 convolutions of its four blocks (conv1, conv3 and, at stride 1, the shortcut): 32 -> 32, 32 -> 16, 32 -> 16 |
# 16 -> 96, 96 -> 24 | 24 -> 144, 144 -> 24, 24 -> 24 | 24 -> 144, 144 -> 320: ten, none with both counts multiples of 64; the head's
# 320 -> 1280 stays on alignq_qconv_fwd
N_POINTWISE, N_GEMM = 10, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def bits4():
    from alignq_amd import config
    old = (config.args.bitW, config.args.abitW, config.args.act_range, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 4
    config.args.act_range = 2.0
    yield
    (config.args.bitW, config.args.abitW, config.args.act_range, config.args.train_batch_size, config.args.eval_batch_size) = old


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
    w = torch.round(torch.tanh(torch.randn(cout, cin, 1, 1, generator=g)) * n) / n
    return w.to(dev).contiguous(memory_format=CL)


def _bar(got, ref64, torch32, what):
    """tests/test_gpu_qconv.py::_check's bar: no further from the fp64 result than torch's own fp32 convolution on the same inputs, or
    2e-6 of the largest fp64 magnitude"""
    floor = 2e-6 * float(ref64.abs().max())
    err, err32 = float((got.double() - ref64).abs().max()), float((torch32.double() - ref64).abs().max())
    print("%s: max err %.3e, torch fp32 %.3e, floor %.3e" % (what, err, err32, floor))
    assert err <= max(err32, floor), (what, err, err32, floor)


def _check_layer(x, wq, gy, y, dx, dw, what):
    """y, dx, dw of one layer against fp64 on its own inputs"""
    xd, wd = x.detach().double().requires_grad_(True), wq.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd)
    yd.backward(gy.double())
    y32 = F.conv2d(x.detach(), wq.detach())
    dx32, dw32 = torch.ops.aten.convolution_backward(gy, x.detach(), wq.detach(), None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
                                                     (True, True, False))[:2]
    _bar(y.detach(), yd.detach(), y32, what + " fwd")
    _bar(dx, xd.grad, dx32, what + " dgrad")
    _bar(dw, wd.grad, dw32, what + " wgrad")


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("cin,cout,B,H", SHAPES)
def test_qconv_pw_matches_fp64(dev, cin, cout, B, H, k):
    from alignq_amd import ops
    seed = cin + 3 * cout + H + k
    wq = _wq(cout, cin, k, dev, seed).requires_grad_(True)
    x = (torch.randn(B, cin, H, H, generator=torch.Generator().manual_seed(seed + 1)) * 1.3).to(dev).contiguous(memory_format=CL)
    x.requires_grad_(True)
    assert ops.qconv_pw_supported(x, wq, (1, 1), (0, 0), (1, 1), 1, None, k)
    y = ops.QConvPwFn.apply(x, wq, k)
    assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (B, cout, H, H)
    gy = (torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 2)) * 1e-3).to(dev).contiguous(memory_format=CL)
    y.backward(gy)
    _check_layer(x, wq, gy, y, x.grad, wq.grad, "%d->%d k=%d" % (cin, cout, k))


def test_backward_honours_needs_input_grad(dev, monkeypatch):
    from alignq_amd import ops
    calls = count_calls(monkeypatch, "alignq_pwconv_dgrad", "alignq_pwconv_wgrad")
    wq = _wq(24, 16, 4, dev, 1)
    x = torch.randn(2, 16, 3, 3, device=dev).contiguous(memory_format=CL)
    gy = torch.randn(2, 24, 3, 3, device=dev)                                  # not channels-last: made so by the backward
    ops.QConvPwFn.apply(x.clone().requires_grad_(True), wq, 4).backward(gy)
    assert calls == {"alignq_pwconv_dgrad": 1, "alignq_pwconv_wgrad": 0}
    ops.QConvPwFn.apply(x, wq.clone().requires_grad_(True), 4).backward(gy)
    assert calls == {"alignq_pwconv_dgrad": 1, "alignq_pwconv_wgrad": 1}


def pointwise_layers(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1)
            and (m.in_channels % 64 or m.out_channels % 64)]


def test_pointwise_layers_in_situ(dev, monkeypatch, bits4):
    """The REDUCED_CFG model at 4W/4A, one forward and backward with use_hip_convs(net, pointwise=True): every eligible layer goes
    through alignq_pwconv_fwd and is held, on its own captured inputs, to the bar above; 320 -> 1280 stays on alignq_qconv_fwd; all
    parameter gradients are finite; a second identical iteration gives bit-equal gradients on the pointwise filters."""
    from alignq_amd import mobilenet as M
    calls = count_calls(monkeypatch, PW_FWD, GEMM_FWD)
    monkeypatch.setattr(M.MobileNetV2, "cfg", list(REDUCED_CFG))
    net = M.use_hip_convs(mobilenet_init_(M.mobile_v2(4, 4, "no_align")).to(dev), pointwise=True).train()
    layers = pointwise_layers(net)
    assert len(layers) == N_POINTWISE
    rec = [dict() for _ in layers]

    def attach(conv, r):
        def pre(mod, inp):
            alias = inp[0].view_as(inp[0])          # this consumer's own edge: a block's input also feeds its shortcut convolution
            r["x"] = alias
            alias.register_hook(lambda g: r.__setitem__("dx", g))
            return (alias,)

        def post(mod, inp, res):
            r["y"] = res
            res.register_hook(lambda g: r.__setitem__("dy", g))

        def wq(mod, inp, res):
            res.retain_grad()
            r["wq"] = res
        conv.register_forward_pre_hook(pre)
        conv.register_forward_hook(post)
        conv.quantize_fn.register_forward_hook(wq)
    for conv, r in zip(layers, rec):
        attach(conv, r)
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(dev).contiguous(memory_format=CL)
    target = torch.tensor([1, 3, 5, 7], device=dev)

    def iteration():
        net.zero_grad(set_to_none=True)
        logits = net(x)
        snap = [{k: v.detach().clone() for k, v in r.items()} for r in rec]       # before the in-place shortcut adds
        F.cross_entropy(logits, target).backward()
        return snap
    snap = iteration()
    assert calls == {PW_FWD: N_POINTWISE, GEMM_FWD: N_GEMM}
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    for conv, r, f in zip(layers, rec, snap):
        assert f["x"].is_contiguous(memory_format=CL)
        _check_layer(f["x"], f["wq"], r["dy"].contiguous(memory_format=CL), f["y"], r["dx"], r["wq"].grad,
                     "%d->%d" % (conv.in_channels, conv.out_channels))
    first = [(r["wq"].grad.clone(), conv.weight.grad.clone()) for conv, r in zip(layers, rec)]
    iteration()
    assert calls == {PW_FWD: 2 * N_POINTWISE, GEMM_FWD: 2 * N_GEMM}
    for (gq, gw), conv, r in zip(first, layers, rec):
        assert torch.equal(gq.view(torch.int32), r["wq"].grad.view(torch.int32)), "dW_q differs between two identical iterations"
        assert torch.equal(gw.view(torch.int32), conv.weight.grad.view(torch.int32)), "dW differs between two identical iterations"


def test_default_is_off(dev, monkeypatch, bits4):
    """use_hip_convs(net) alone: the new forward entry point is never called, in training or inside EvalStep"""
    from alignq_amd import mobilenet as M
    from alignq_amd.eval_step import EvalStep
    calls = count_calls(monkeypatch, PW_FWD, GEMM_FWD)
    monkeypatch.setattr(M.MobileNetV2, "cfg", list(REDUCED_CFG))
    net = M.use_hip_convs(mobilenet_init_(M.mobile_v2(4, 4, "no_align")).to(dev)).train()
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(dev).contiguous(memory_format=CL)
    F.cross_entropy(net(x), torch.tensor([1, 3, 5, 7], device=dev)).backward()
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        ev(x, torch.tensor([1, 3, 5, 7], device=dev))
    assert calls == {PW_FWD: 0, GEMM_FWD: 2 * N_GEMM}


def test_eval_step_with_pointwise_on_g20(dev, monkeypatch, bits4):
    """EvalStep on fixture G20 with pointwise=True: the two assertions of test_eval_step_against_reference_network_g20 (the reference's
    precision counts; logits within twice the error of this repository's own `model.eval()` forward, measured before the opt-in), the
    captured replay equal to the eager batch bit for bit, the same logits from weights=pack_model(net), the state_dict untouched, and
    the filter bins packed during begin(), never during a batch."""
    from alignq_amd import export
    from alignq_amd import mobilenet as M
    from alignq_amd.eval_step import EvalStep
    g = load_golden("g20_mobilenet_eval")
    B = int(g["batch"])
    assert int(g["bits"]) == 4 and float(g["act_range"]) == 2.0
    net = reduced_net(monkeypatch, dev, str(g["stage"]), g)
    x = torch.from_numpy(g["x"]).to(dev).contiguous(memory_format=CL)
    y = torch.from_numpy(g["targets"]).to(dev)
    parent = bare_eval(net, x).cpu().numpy()
    net = M.use_hip_convs(net, pointwise=True)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    calls = count_calls(monkeypatch, PW_FWD, GEMM_FWD, PACK)
    ev = EvalStep(net, channels_last=True, qconv=True)
    with ev:
        assert calls[PACK] >= 1 and calls[PW_FWD] == 0           # begin() packed the bins of every filter
        packed = calls[PACK]
        eager = ev(x, y).clone()
        ce, prec1, prec5, n = ev.result()
        assert calls == {PW_FWD: N_POINTWISE, GEMM_FWD: N_GEMM, PACK: packed}          # no pack launch per batch and layer
    logits = eager.cpu().numpy()
    ref, min_margin = g["logits"], float(g["min_margin"])
    err_parent, err_new = float(np.abs(parent - ref).max()), float(np.abs(logits - ref).max())
    print("G20 pointwise: max |logits - reference| EvalStep %.3e, model.eval() %.3e (min_margin %.3e); ce %.6f (reference %.6f); "
          "Prec@1 %.4f (%.4f) Prec@5 %.4f (%.4f)" % (err_new, err_parent, min_margin, ce, float(g["ce"]), prec1, float(g["prec1"]),
                                                     prec5, float(g["prec5"])))
    assert 2.0 * err_new < min_margin, "fixture problem: G20's targets are not far enough from the rank boundaries for this error"
    assert n == B
    assert round(prec1 * B / 100.0) == round(float(g["prec1"]) * B / 100.0)
    assert round(prec5 * B / 100.0) == round(float(g["prec5"]) * B / 100.0)
    assert err_new <= max(2.0 * err_parent, 1e-5)
    # captured: the recording makes the new launches (and no pack launch); the replay makes no call from the host at all
    with ev:
        packed = calls[PACK]
        ev.capture(x, y, warmup=1)
        recorded = dict(calls)
        assert recorded[PW_FWD] == 3 * N_POINTWISE and recorded[PACK] == packed          # eager batch + warm-up + recording
        cap = ev(x, y).clone()
        assert ev._graph is not None and calls == recorded
    assert torch.equal(cap.view(torch.int32), eager.view(torch.int32)), "captured replay differs from the eager batch"
    after = net.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    # from the packed codes: the unpack launch emits the bins; the fp32 filters are never read
    pk = export.pack_model(net)
    skeleton = M.use_hip_convs(M.mobile_v2(4, 4, str(g["stage"])).to(dev), pointwise=True)
    pk.apply(skeleton)
    with torch.no_grad():
        for name, c in export.quantised_convs(skeleton):
            c.weight.fill_(float("nan"))
    for k in calls:
        calls[k] = 0
    with EvalStep(skeleton, weights=pk) as ev2:
        got = ev2(x, y).clone()
    assert calls == {PW_FWD: N_POINTWISE, GEMM_FWD: N_GEMM, PACK: 0}
    assert torch.equal(got.view(torch.int32), eager.view(torch.int32)), "logits from the packed weights differ"
