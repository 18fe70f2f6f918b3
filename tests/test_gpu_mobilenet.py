"""MobileNet-V2 (alignq_amd/mobilenet.py) on the GPU: the depthwise layers against fixture G19 (b) (captured from the reference's
cdf_alignment/mobilenet-v2-svhn/model/mobilenetV2.py on CPU), the whole network's wiring against G19 (c), every depthwise layer
inside a 4W/4A forward + backward against tests/dwconv_oracle.py, and one eager training iteration of the full model."""
import numpy as np
import pytest
import torch

from tests import dwconv_oracle as D
from tests.conftest import load_golden
from tests.golden.mobilenet_init import REDUCED_CFG, mobilenet_init_

pytestmark = pytest.mark.gpu

CL = torch.channels_last
FWD = "alignq_dwconv3x3_nhwc_fwd"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_mobilenet")


@pytest.fixture
def bits4():
    from alignq_amd import config
    old = (config.args.bitW, config.args.abitW)
    config.args.bitW = config.args.abitW = 4
    yield
    config.args.bitW, config.args.abitW = old


def count_forwards(monkeypatch):
    from alignq_amd import _lib as L
    lib = L.load()
    calls = [0]
    orig = getattr(lib, FWD)

    def wrapper(*a):
        calls[0] += 1
        return orig(*a)
    monkeypatch.setattr(lib, FWD, wrapper)
    return calls


def depthwise_layers(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]


@pytest.mark.parametrize("i", range(4))
def test_fixture_depthwise_layers(dev, g19, monkeypatch, i):
    import alignq_amd.cdf_alignment as A
    calls = count_forwards(monkeypatch)
    w, x, dy, s = g19[f"dw{i}_w"], g19[f"dw{i}_x"], g19[f"dw{i}_dy"], int(g19[f"dw{i}_stride"])
    C, (H, W) = w.shape[0], x.shape[2:]
    conv = A.conv2d_Q_fn(4, str(g19["stage"]))(C, C, 3, s, 1, groups=C, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
    conv.use_qconv = True
    held = {}

    def keep(mod, inp, res):
        res.retain_grad()
        held["wq"] = res
    conv.quantize_fn.register_forward_hook(keep)
    xt = torch.from_numpy(x).to(dev).contiguous(memory_format=CL).requires_grad_(True)
    y = conv(xt)
    y.backward(torch.from_numpy(dy).to(dev))
    assert calls[0] == 1
    wq = held["wq"]
    n_diff = int((wq.detach().cpu().numpy() != g19[f"dw{i}_wq"]).sum())
    assert n_diff == 0, f"{n_diff} of {wq.numel()} quantised levels differ from the reference's"
    ref_wq = g19[f"dw{i}_wq"]
    for name, got, want, bound in (
            ("y", y, g19[f"dw{i}_y"], D.fwd_bound(x, ref_wq, s)),
            ("dx", xt.grad, g19[f"dw{i}_dx"], D.dgrad_bound(dy, ref_wq, s, H, W)),
            ("dwq", wq.grad, g19[f"dw{i}_dwq"], D.wgrad_bound(x, dy, s).reshape(C, 1, 3, 3))):
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
        print(f"layer {i} {name}: max err {err.max():.3e}, max err / (2 bound) {(err / np.maximum(2 * bound, 1e-300)).max():.3e}")
        assert (err <= 2 * bound).all(), name             # two fp32 evaluations of the same sums: the bound doubles
    assert torch.isfinite(conv.weight.grad).all()


def reduced(monkeypatch, wbit, abit, stage):
    from alignq_amd import mobilenet as M
    monkeypatch.setattr(M.MobileNetV2, "cfg", list(REDUCED_CFG))
    return M.mobile_v2(wbit, abit, stage)


def test_fixture_wiring_32_bits(dev, g19, monkeypatch):
    from alignq_amd import mobilenet as M
    calls = count_forwards(monkeypatch)
    net = M.use_hip_convs(mobilenet_init_(reduced(monkeypatch, 32, 32, str(g19["stage"]))).to(dev)).train()
    x = torch.from_numpy(g19["c_x"]).to(dev).contiguous(memory_format=CL)
    logits = net(x).detach().cpu().numpy().astype(np.float64)
    e_ref = float(g19["c_e_ref"])
    err = float(np.abs(logits - g19["c_logits64"]).max())
    print(f"wiring: max |logits - logits64| {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert calls[0] == 4 == len(depthwise_layers(net))
    assert err <= 8 * e_ref
    assert tuple(net.out.shape) == (4, 1280, 1, 1)


def test_depthwise_layers_in_situ(dev, monkeypatch, bits4):
    from alignq_amd import mobilenet as M
    calls = count_forwards(monkeypatch)
    net = M.use_hip_convs(mobilenet_init_(reduced(monkeypatch, 4, 4, "no_align")).to(dev)).train()
    layers = depthwise_layers(net)
    assert len(layers) == 4
    rec = [dict() for _ in layers]

    def attach(conv, r):
        def pre(mod, inp):
            r["x"] = inp[0]
            inp[0].register_hook(lambda g: r.__setitem__("dx", g))

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
    logits = net(x)
    snap = [{k: v.detach().cpu().numpy().copy() for k, v in r.items()} for r in rec]       # before the in-place shortcut adds
    torch.nn.functional.cross_entropy(logits, torch.tensor([1, 3, 5, 7], device=dev)).backward()
    assert calls[0] == len(layers)
    for conv, r, f in zip(layers, rec, snap):
        s = conv.stride[0]
        xi, wq, dy = f["x"], f["wq"], r["dy"].cpu().numpy()
        H, W = xi.shape[2:]
        assert D.bits_equal(f["y"], D.fwd32(xi, wq, s))
        assert D.bits_equal(r["dx"].cpu().numpy(), D.dgrad32(dy, wq, s, H, W))
        err = np.abs(r["wq"].grad.cpu().numpy().reshape(-1, 3, 3) - D.wgrad64(xi, dy, s))
        assert (err <= D.wgrad_bound(xi, dy, s)).all()
        assert (xi == 0).mean() > 0.05           # the real inputs: ReLU6 of quantised levels, many exact zeros


def test_one_eager_training_iteration(dev, bits4):
    from alignq_amd import mobilenet as M
    from alignq_amd.cdf_alignment import SGD
    net = M.use_hip_convs(mobilenet_init_(M.mobile_v2(4, 4, "no_align")).to(dev)).train()
    twin = mobilenet_init_(M.mobile_v2(4, 4, "no_align")).to(dev).to(memory_format=CL).train()       # use_qconv off
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(dev).contiguous(memory_format=CL)
    target = torch.tensor([0, 2, 4, 6], device=dev)
    before = [p.detach().clone() for p in net.parameters()]
    opt = SGD(net.parameters(), lr=0.04, momentum=0.9, weight_decay=2e-4)
    opt.zero_grad()
    logits = net(x)
    torch.nn.functional.cross_entropy(logits, target).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    opt.step([], [], [], 1.0, 4.0)
    torch.cuda.synchronize()
    unchanged = [n for (n, p), b in zip(net.named_parameters(), before) if torch.equal(p.detach(), b)]
    assert not unchanged, unchanged
    assert tuple(twin(x).shape) == tuple(logits.shape) == (4, 10)
