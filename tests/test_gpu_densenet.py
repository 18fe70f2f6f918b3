"""DenseNet (alignq_amd/densenet.py) on the GPU: four dense layers against fixture G21 (b) (captured from the reference's
cdf_alignment/dense-cifar-10/model/densenet.py on CPU), the whole network's wiring against G21 (c), every dense layer inside a 4W/4A
forward + backward with densenet.use_hip_convs held to the fp64 bar on its own captured inputs, the default (flag off), and two eager
training iterations."""
import numpy as np
import pytest
import torch

from tests import weights_oracle as WO
from tests.conftest import load_golden
from tests.golden.densenet_init import REDUCED, TF_LAYERS, densenet_init_
from tests.test_gpu_k3conv import bar, check_layer, count_calls

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F = torch.nn.functional
K3_FWD, PW_FWD = "alignq_k3conv_fwd", "alignq_pwconv_fwd"
N_DENSE, N_TRANS = 6, 2          # REDUCED: 3x3 layers 24, 36 | 48, 60 | 72, 84 -> 12; transitions 48 -> 48 and 72 -> 72


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_densenet")


@pytest.fixture
def bits4():
    from alignq_amd import config
    old = (config.args.bitW, config.args.abitW, config.args.act_range)
    config.args.bitW = config.args.abitW = 4
    config.args.act_range = 2.0
    yield
    config.args.bitW, config.args.abitW, config.args.act_range = old


@pytest.mark.parametrize("i", range(4))
def test_fixture_dense_layers(dev, g21, monkeypatch, i):
    """y, dx, dW_q and dW of one dense layer from the fixture's own x, raw filter and dy: no further from fp64 than the reference's own
    fp32 results in the fixture (or 2e-6 of the largest magnitude); the quantised levels equal the reference's exactly"""
    from alignq_amd import densenet as D
    calls = count_calls(monkeypatch, K3_FWD, "alignq_k3conv_dgrad", "alignq_k3conv_wgrad")
    w, x, dy = g21[f"k{i}_w"], g21[f"k{i}_x"], g21[f"k{i}_dy"]
    cin = w.shape[1]
    assert TF_LAYERS[i][0] in ("dense1", "dense2", "dense3") and float(g21["act_range"]) == 2.0
    conv = D.conv2d_Q3_fn(4, str(g21["stage"]))(cin, 12, kernel_size=3, padding=1, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
    conv = conv.to(memory_format=CL)
    conv.use_qconv = conv.use_qconv_k3 = True
    held = {}

    def keep(mod, inp, res):
        res.retain_grad()
        held["wq"] = res
    conv.quantize_fn.register_forward_hook(keep)
    xt = torch.from_numpy(x).to(dev).contiguous(memory_format=CL).requires_grad_(True)
    y = conv(xt)
    y.backward(torch.from_numpy(dy).to(dev))
    assert calls == {K3_FWD: 1, "alignq_k3conv_dgrad": 1, "alignq_k3conv_wgrad": 1}
    wq = held["wq"]
    n_diff = int((wq.detach().cpu().numpy() != g21[f"k{i}_wq"]).sum())
    assert n_diff == 0, f"{n_diff} of {wq.numel()} quantised levels differ from the reference's"
    # fp64 on the fixture's inputs; the filter gradient goes on through the float64 statement of the quantiser's backward
    xd = torch.from_numpy(x).double().requires_grad_(True)
    wd = torch.from_numpy(g21[f"k{i}_wq"]).double().requires_grad_(True)
    yd = F.conv2d(xd, wd, None, 1, 1)
    yd.backward(torch.from_numpy(dy).double())
    m, s = WO.weight_stats64(w)
    dw64 = torch.from_numpy(WO.weight_quant_bwd64(wd.grad.numpy(), w, m, s).reshape(w.shape))
    for name, got, ref64, ref32 in (("y", y, yd.detach(), g21[f"k{i}_y"]), ("dx", xt.grad, xd.grad, g21[f"k{i}_dx"]),
                                    ("dW_q", wq.grad, wd.grad, g21[f"k{i}_dwq"]), ("dW", conv.weight.grad, dw64, g21[f"k{i}_dw"])):
        bar(got.detach().cpu(), ref64, torch.from_numpy(ref32), "layer %d %s" % (i, name))


def test_fixture_wiring_32_bits(dev, g21, monkeypatch):
    from alignq_amd import densenet as D
    net = D.use_hip_convs(densenet_init_(D.DenseNet(32, 32, str(g21["stage"]), **REDUCED)).to(dev)).train()
    x = torch.from_numpy(g21["c_x"]).to(dev).contiguous(memory_format=CL)
    logits = net(x).detach().cpu().numpy().astype(np.float64)
    e_ref = float(g21["c_e_ref"])
    err = float(np.abs(logits - g21["c_logits64"]).max())
    print(f"wiring: max |logits - logits64| {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert err <= 8 * e_ref


def dense_layers(net):
    return [blk.conv1 for stage in (net.dense1, net.dense2, net.dense3) for blk in stage]


def test_dense_layers_in_situ(dev, monkeypatch, bits4):
    """The reduced model at 4W/4A, one forward and backward with use_hip_convs: every dense layer goes through alignq_k3conv_fwd (the
    concatenations stay channels-last) and is held, on its own captured inputs, to the fp64 bar; both transitions go through
    alignq_pwconv_fwd; all parameter gradients are finite; a second identical iteration gives bit-equal gradients on the six filters."""
    from alignq_amd import densenet as D
    calls = count_calls(monkeypatch, K3_FWD, PW_FWD)
    net = D.use_hip_convs(densenet_init_(D.DenseNet(4, 4, "no_align", **REDUCED)).to(dev)).train()
    layers = dense_layers(net)
    assert len(layers) == N_DENSE and [c.in_channels for c in layers] == [24, 36, 48, 60, 72, 84]
    rec = [dict() for _ in layers]

    def attach(conv, r):
        def pre(mod, inp):
            alias = inp[0].view_as(inp[0])          # this consumer's own edge
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
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev).contiguous(memory_format=CL)
    target = torch.tensor([1, 3, 5, 7], device=dev)

    def iteration():
        net.zero_grad(set_to_none=True)
        logits = net(x)
        snap = [{k: v.detach().clone() for k, v in r.items()} for r in rec]
        F.cross_entropy(logits, target).backward()
        return snap
    snap = iteration()
    assert calls == {K3_FWD: N_DENSE, PW_FWD: N_TRANS}
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    for conv, r, f in zip(layers, rec, snap):
        assert f["x"].is_contiguous(memory_format=CL) and f["y"].is_contiguous(memory_format=CL)
        assert float((f["x"] == 0).float().mean()) > 0.05           # the real inputs: ReLU of quantised levels, many exact zeros
        check_layer(f["x"], f["wq"], r["dy"].contiguous(memory_format=CL), f["y"], r["dx"], r["wq"].grad,
                    "%d->%d" % (conv.in_channels, conv.out_channels))
    first = [(r["wq"].grad.clone(), conv.weight.grad.clone()) for conv, r in zip(layers, rec)]
    iteration()
    assert calls == {K3_FWD: 2 * N_DENSE, PW_FWD: 2 * N_TRANS}
    for (gq, gw), conv, r in zip(first, layers, rec):
        assert torch.equal(gq.view(torch.int32), r["wq"].grad.view(torch.int32)), "dW_q differs between two identical iterations"
        assert torch.equal(gw.view(torch.int32), conv.weight.grad.view(torch.int32)), "dW differs between two identical iterations"


def test_default_is_off(dev, monkeypatch, bits4):
    """channels-last parameters and `use_qconv` alone: the new entry point is never called"""
    from alignq_amd import densenet as D
    from alignq_amd import paths
    calls = count_calls(monkeypatch, K3_FWD, PW_FWD)
    net = densenet_init_(D.DenseNet(4, 4, "no_align", **REDUCED)).to(dev).to(memory_format=CL).train()
    paths.apply(net, use_qconv=True)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev).contiguous(memory_format=CL)
    logits = net(x)
    F.cross_entropy(logits, torch.tensor([1, 3, 5, 7], device=dev)).backward()
    assert calls == {K3_FWD: 0, PW_FWD: 0} and bool(torch.isfinite(logits).all())


def test_two_eager_training_iterations(dev, bits4):
    """depth 16 (3x3 layers of 24 ... 156 channels, transitions 72 -> 72 and 120 -> 120): the 40-layer model's loop at a third of its
    launches"""
    from alignq_amd import densenet as D
    from alignq_amd.optimizer import SGD
    net = D.use_hip_convs(densenet_init_(D.DenseNet(4, 4, "no_align", depth=16, compressionRate=1)).to(dev)).train()
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(dev).contiguous(memory_format=CL)
    target = torch.tensor([0, 2, 4, 6], device=dev)
    opt = SGD(net.parameters(), lr=0.04, momentum=0.9, weight_decay=2e-4)
    losses = []
    for _ in range(2):
        before = [p.detach().clone() for p in net.parameters()]
        opt.zero_grad()
        logits = net(x)
        loss = F.cross_entropy(logits, target)
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        opt.step([], [], [], 1.0, 4.0)
        torch.cuda.synchronize()
        losses.append(float(loss.detach()))
        unchanged = [n for (n, p), b in zip(net.named_parameters(), before) if torch.equal(p.detach(), b)]
        assert not unchanged, unchanged
    assert tuple(logits.shape) == (4, 10) and all(np.isfinite(losses)), losses
