"""The digit-domain DANN (alignq_amd/digit.py) on the GPU: one eager training iteration at 4W/4A (source batch + target batch) with
digit.use_hip_convs, every Conv2d_Q5 call held to the fp64 bar of tests/test_gpu_k3conv.py on its OWN inputs (teacher-forced: whole-
network outputs are not compared across paths, a last-bit difference can move a quantiser level downstream), and the default (flag
off).  Reference: cdf_alignment/dann_digit/model/dann.py:125-230, main.py:355-372."""
import pytest
import torch

from tests.golden.digit_init import digit_init_
from tests.test_gpu_k3conv import bar, count_calls

pytestmark = pytest.mark.gpu

F = torch.nn.functional
K5 = ("alignq_k5conv_fwd", "alignq_k5conv_dgrad", "alignq_k5conv_wgrad")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def bits4():
    from alignq_amd import config
    old = (config.args.bitW, config.args.abitW, config.args.act_range)
    config.args.bitW = config.args.abitW = 4
    config.args.act_range = 2.0
    yield
    config.args.bitW, config.args.abitW, config.args.act_range = old


def _iteration(dev, hip):
    from alignq_amd import digit
    from alignq_amd.optimizer import SGD
    torch.manual_seed(5)
    net = digit_init_(digit.MNISTmodel_quant("org", 4, 4)).to(dev).train()
    if hip:
        digit.use_hip_convs(net)
    g = torch.Generator().manual_seed(6)
    src, tgt = torch.randn(4, 1, 28, 28, generator=g).to(dev), torch.randn(4, 3, 28, 28, generator=g).to(dev)
    labels = torch.randint(0, 10, (4,), generator=g).to(dev)
    return net, lambda: digit.train_iteration(net, SGD(net.parameters(), lr=0.01, momentum=0.9), src, labels, tgt, 0.3)


def test_training_iteration_every_k5_call_against_fp64(dev, bits4, monkeypatch):
    calls = count_calls(monkeypatch, *K5)
    net, run = _iteration(dev, True)
    convs = [net.feature[0], net.feature[5]]
    seen = [[], []]          # per layer, per call: {x, wq, y, gy, gx}
    for i, conv in enumerate(convs):
        def pre(mod, inp, i=i):
            rec = {"x": inp[0]}
            if inp[0].requires_grad:
                inp[0].register_hook(lambda g, rec=rec: rec.__setitem__("gx", g))
            seen[i].append(rec)

        def keep_wq(mod, inp, res, i=i):
            res.retain_grad()
            seen[i][-1]["wq"] = res

        def post(mod, inp, res, i=i):
            seen[i][-1]["y"] = res
            res.register_hook(lambda g, rec=seen[i][-1]: rec.__setitem__("gy", g))

        conv.register_forward_pre_hook(pre)
        conv.quantize_fn.register_forward_hook(keep_wq)
        conv.register_forward_hook(post)
    bias_before = [c.bias.detach().clone() for c in convs]
    losses = run()
    assert all(torch.isfinite(v) for v in losses)
    # per iteration: two forwards and two filter gradients per layer, the data gradient of the second layer alone
    assert calls == {K5[0]: 4, K5[1]: 2, K5[2]: 4}
    for i, conv in enumerate(convs):
        assert len(seen[i]) == 2
        db64, db32 = 0.0, 0.0
        for c, rec in enumerate(seen[i]):
            x, wq, gy = rec["x"].detach(), rec["wq"].detach(), rec["gy"]
            want_dx = i == 1
            xd, wd, bd = x.double().requires_grad_(want_dx), wq.double().requires_grad_(True), bias_before[i].double()
            yd = F.conv2d(xd, wd, bd)
            yd.backward(gy.double())
            dx32, dw32 = torch.ops.aten.convolution_backward(gy, x, wq, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
                                                             (want_dx, True, False))[:2]
            what = "layer %d call %d " % (i, c)
            bar(rec["y"].detach(), yd.detach(), F.conv2d(x, wq, bias_before[i]), what + "y")
            bar(rec["wq"].grad, wd.grad, dw32, what + "dw")
            if want_dx:
                bar(rec["gx"], xd.grad, dx32, what + "dx")
            db64, db32 = db64 + gy.double().sum((0, 2, 3)), db32 + gy.sum((0, 2, 3))
        bar(conv.bias.grad, db64, db32, "layer %d dbias" % i)


def test_flag_off_takes_no_k5_call(dev, bits4, monkeypatch):
    calls = count_calls(monkeypatch, *K5)
    net, run = _iteration(dev, False)
    assert all(torch.isfinite(v) for v in run())
    assert calls == dict.fromkeys(K5, 0)
