"""GPU checks of the evaluation pass (include/alignq.h: alignq_bnq_eval_fwd, alignq_eval_metrics; alignq_amd/eval_step.py).

Kernel against the C oracle: a, b and x = a z + b are restated in NumPy fp32 with the arithmetic the header states (every
operation rounded on its own); the quantiser's expected output comes from oracle/alignq_oracle.c (`oracle_c.bn_site_fwd` for the
ADMM formula, `oracle_c.bn_apply` + `oracle_c.act_quant_fwd` for the CDF formula, both fed x through the identity coefficients
a = 1, b = 0, for which their fmaf(a, x, b) returns x itself).  y and the packed indices must be bit-identical.  The oracle runs
once per (shape, formula, k) without residual and ReLU; `+ residual` and `v > 0 ? v : 0` are then the same two IEEE operations in
NumPy as in the oracle (checked against the oracle's own residual / ReLU arguments on the small shapes)."""
import itertools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests.conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import eval_inputs as E  # noqa: E402
from eval_inputs import ab_numpy, metrics_numpy  # noqa: E402

pytestmark = pytest.mark.gpu

ADMM, CDF = 0, 1
R = 2.0
SHAPES = [(100, 16, 32, 32), (100, 64, 8, 8), (28, 256, 56, 56), (28, 2048, 7, 7),
          (7, 32, 16, 16),            # a short last batch
          (2, 2048, 128, 64)]         # 2^25 elements: the non-temporal branch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def site_inputs(shape, seed):
    """z, residual in channels-last memory order [B, H, W, C] and the batch-norm vectors (running statistics away from (0, 1))"""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, H, W, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    res = rng.standard_normal((B, H, W, C), dtype=np.float32)
    gamma = (0.5 + rng.random(C)).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
    mean = (rng.standard_normal(C) * 0.5 + 0.2).astype(np.float32)
    var = (0.3 + 2.0 * rng.random(C)).astype(np.float32)
    return z, res, gamma, beta, mean, var


def launch(dev, z_t, C, vecs, k, r, formula, relu, res_t, pack, both=False):
    from alignq_amd import _lib as L
    lib = L.load()
    g, b, m, v = vecs
    P = z_t.numel() // C
    y = torch.empty_like(z_t) if (not pack or both) else None
    bins = torch.empty(z_t.shape, dtype=torch.int8 if pack == 1 else torch.int16, device=dev) if pack else None
    rc = lib.alignq_bnq_eval_fwd(L.ptr(z_t), P, C, L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), 1e-5, k, r, formula, int(relu),
                                 L.ptr(res_t), L.ptr(y), L.ptr(bins), pack, L.stream_ptr())
    return rc, y, bins


def post(xq, res, relu):
    v = xq if res is None else (xq + res).astype(np.float32)
    return np.where(v > 0, v, np.float32(0.0)).astype(np.float32) if relu else v


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bnq_eval_kernel_bit_identical_to_c_oracle(dev, shape):
    from alignq_amd import _lib as L
    lib = L.load()
    B, C, H, W = shape
    z, res, gamma, beta, mean, var = site_inputs(shape, 1000 + C + B)
    a, b = ab_numpy(gamma, beta, mean, var, 1e-5)
    cidx = np.arange(C)
    x = ((a[cidx] * z).astype(np.float32) + b[cidx]).astype(np.float32)          # channel = element index mod C
    ident = np.stack([np.ones(C, np.float32), np.zeros(C, np.float32)])
    x2 = x.reshape(B, -1)
    assert np.array_equal(bits(O.bn_apply(x2, C, 1, ident)), bits(x2))
    z_t, res_t = torch.from_numpy(z).to(dev), torch.from_numpy(res).to(dev)
    vecs = tuple(torch.from_numpy(t).to(dev) for t in (gamma, beta, mean, var))
    small = z.size <= (1 << 21)
    n_checked = 0
    for formula, k in itertools.product((ADMM, CDF), (2, 4, 8, 32)):
        idx = None
        if k == 32:
            xq = x2                                                        # no quantiser: the batch-norm alone
        elif formula == ADMM:
            xq, _, _ = O.bn_site_fwd(x2, C, 1, ident, k, R)
            oq, _, idx = O.act_quant_fwd(x2, k, R, ADMM)                     # the level indices; ties the two oracle entry points
            assert np.array_equal(bits(xq), bits(oq))
        else:
            xq, _, _ = O.act_quant_fwd(O.bn_apply(x2, C, 1, ident), k, R, CDF)
        xq = xq.reshape(z.shape)
        for relu, with_res, packed in itertools.product((False, True), (False, True), (False, True)):
            nb = lib.alignq_bin_bytes(k, R, ADMM) if k != 32 else 0
            pack = (nb if nb else 1) if packed else 0
            rc, y, bins = launch(dev, z_t, C, vecs, k, R, formula, relu, res_t if with_res else None, pack)
            if packed and (formula != ADMM or with_res or k == 32):
                assert rc == L.EINVAL, (formula, k, relu, with_res, rc)      # no packed form: refused before any launch
                continue
            assert rc == 0, (formula, k, relu, with_res, packed, rc)
            if packed:
                exp = (np.maximum(idx, 0) if relu else idx).reshape(z.shape)
                exp_t = torch.from_numpy(exp.astype(np.int8 if nb == 1 else np.int16)).to(dev)
                assert torch.equal(bins, exp_t), (formula, k, relu)
                # fp32 y TOGETHER with the indices (the header allows both outputs): the same indices, and the fp32 values
                rc, y2, bins2 = launch(dev, z_t, C, vecs, k, R, formula, relu, None, pack, both=True)
                assert rc == 0 and torch.equal(bins2, exp_t)
                exp_y = torch.from_numpy(post(xq, None, relu)).to(dev)
                assert torch.equal(y2.view(torch.int32), exp_y.view(torch.int32)), (formula, k, relu, "y beside the indices")
            else:
                exp = post(xq, res if with_res else None, relu)
                if small and formula == ADMM and k != 32:                    # the oracle's own residual / ReLU arguments
                    oy, _, _ = O.bn_site_fwd(x2, C, 1, ident, k, R, residual=res.reshape(B, -1) if with_res else None, relu=relu)
                    assert np.array_equal(bits(oy.reshape(z.shape)), bits(exp))
                exp_t = torch.from_numpy(exp).to(dev)
                same = torch.equal(y.view(torch.int32), exp_t.view(torch.int32))
                if not same:
                    bad = int((y.view(torch.int32) != exp_t.view(torch.int32)).sum())
                    raise AssertionError(f"{bad} of {z.size} elements differ: formula={formula} k={k} relu={relu} res={with_res}")
            n_checked += 1
    assert n_checked == 2 * 4 * 4 + 3 * 2        # every fp32 combination + the packed ones that exist (ADMM, k in 2 4 8, relu on/off)


def test_bnq_eval_office_act_range_and_defaults(dev):
    """act_range = 1 (an Office configuration) and a batch-norm without affine parameters (gamma = 1, beta = 0)"""
    from alignq_amd import _lib as L
    shape = (5, 64, 7, 7)
    B, C, H, W = shape
    z, res, gamma, beta, mean, var = site_inputs(shape, 77)
    one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
    a, b = ab_numpy(one, zero, mean, var, 1e-5)
    x = ((a * z).astype(np.float32) + b).astype(np.float32).reshape(B, -1)
    ident = np.stack([one, zero])
    z_t, res_t = torch.from_numpy(z).to(dev), torch.from_numpy(res).to(dev)
    m_t, v_t = torch.from_numpy(mean).to(dev), torch.from_numpy(var).to(dev)
    for k in (4, 8):
        oy, _, _ = O.bn_site_fwd(x, C, 1, ident, k, 1.0, residual=res.reshape(B, -1), relu=True)
        rc, y, _ = launch(dev, z_t, C, (None, None, m_t, v_t), k, 1.0, ADMM, True, res_t, 0)
        assert rc == 0
        assert np.array_equal(bits(y.cpu().numpy()), bits(oy.reshape(z.shape)))
    rc, _, _ = launch(dev, torch.zeros(2, 3, 3, 12, device=dev), 12, (None, None, m_t, v_t), 4, 1.0, ADMM, True, None, 0)
    assert rc == L.EUNSUPPORTED


# ------------------------------------------------------------------------------------------------ metrics
def run_metrics(dev, batches, K):
    from alignq_amd import _lib as L
    lib = L.load()
    acc = torch.zeros(4, dtype=torch.int64, device=dev)
    for lg, tg in batches:
        lt, tt = torch.from_numpy(lg).to(dev), torch.from_numpy(tg).to(dev)
        L.check(lib.alignq_eval_metrics(L.ptr(lt), L.ptr(tt), lg.shape[0], K, L.ptr(acc), L.stream_ptr()), "alignq_eval_metrics")
    return acc.cpu().numpy()


@pytest.mark.parametrize("K", [10, 31, 1000,
                               1, 4, 5,                        # below 5 classes every valid finite row is a top-5 hit
                               64, 65, 1024])                  # one pass of the 64 lanes, one class more, the largest K
def test_eval_metrics_against_numpy(dev, K):
    rng = np.random.default_rng(K)
    batches = []
    for B in (100, 28, 7,
              1, 2, 4, 5):                                     # the four-row groups' remainders: 1, 2, 0, 1 rows in the last group
        lg = (rng.standard_normal((B, K)) * 3).astype(np.float32)
        tg = rng.integers(0, K, B).astype(np.int64)
        lg[np.arange(0, B, 3), tg[::3]] += 4.0                 # a good share of correct rows
        if B > 1:
            lg[1, (tg[1] + 1) % K] = lg[1, tg[1]]              # a tie with the target: does not count against it
        if B > 3:
            tg[2], tg[3] = -1, K                               # out of range on both sides
        batches.append((lg, tg))
    if K < 5:
        for lg, tg in batches:
            e = metrics_numpy(lg, tg)
            assert e[2] == int(((tg >= 0) & (tg < K)).sum())   # (every valid row is a top-5 hit)
    raw = run_metrics(dev, batches, K)
    exp = [metrics_numpy(lg, tg) for lg, tg in batches]
    ce = float(raw[:1].view(np.float64)[0])
    print("metrics K=%d: ce sum %.9f (numpy %.9f), counts %s" % (K, ce, sum(e[0] for e in exp), raw[1:].tolist()))
    assert raw[1:].tolist() == [sum(e[i] for e in exp) for i in (1, 2, 3)]
    # fp32 expf and per-row log against float64: a few 1e-7 relative per row
    np.testing.assert_allclose(ce, sum(e[0] for e in exp), rtol=2e-6, atol=1e-6 * sum(e[3] for e in exp))
    again = run_metrics(dev, batches, K)
    assert np.array_equal(raw, again)                          # fixed order, no atomics: the same bits
    # NaN rows: counted as wrong, and the cross-entropy sum is NaN as torch's
    lg, tg = batches[0][0].copy(), batches[0][1].copy()
    lg[5, 0] = np.nan
    lg[6, tg[6]] = np.nan
    raw_n = run_metrics(dev, [(lg, tg)], K)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # K = 1: the NaN is the whole row (np.nanmax warns)
        e = metrics_numpy(lg, tg)
    assert raw_n[1:].tolist() == [e[1], e[2], e[3]]
    assert np.isnan(raw_n[:1].view(np.float64)[0])


# ------------------------------------------------------------------------------------------------ EvalStep
def _cifar_net(dev, tree, units, bits_, seed, batch=100):
    from alignq_amd import config
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    from alignq_amd.train_step import TrainStep
    config.args.bitW = config.args.abitW = bits_
    config.args.train_batch_size = 128
    torch.manual_seed(seed)
    net = PreActResNet(PreActBlock_conv_Q, units, bits_, bits_, "second", 10, tree=tree).to(dev).train()
    step = TrainStep(net, channels_last=True, qconv=True)
    x = torch.randn(128, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (128,), device=dev)
    for _ in range(3):
        step(x, y)                       # running statistics away from their initial values
    del x, y
    return net, step


def _state_bits(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same_bits(a, b):
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))
    return torch.equal(a, b)


def _same_state(a, b):
    return a.keys() == b.keys() and all(_same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("tree", ["admm", "cdf"])
def test_eval_step_resnet20_capture_state_and_metrics(dev, tree):
    """ResNet-20 8W/8A at the reference's evaluation batch of 100: EvalStep against the `model.eval()` forward it replaces (the
    bar of test_gpu_parity.test_eval_forward_fast_layout_matches_plain), its accumulated metrics against the NumPy restatement of
    its own logits, captured replay against the eager step bit for bit, the short last batch through the eager path, and an
    untouched state_dict."""
    from alignq_amd import config
    from alignq_amd.eval_step import EvalStep
    try:
        net, _ = _cifar_net(dev, tree, [3, 3, 3], 8, 11)
        g = torch.Generator(device="cpu").manual_seed(3)
        xs = [torch.randn(100, 3, 32, 32, generator=g).to(dev) for _ in range(3)] + [torch.randn(40, 3, 32, 32, generator=g).to(dev)]
        ys = [torch.randint(0, 10, (x.shape[0],), generator=g).to(dev) for x in xs]
        net.eval()
        with torch.no_grad():
            bare = [net(x.contiguous(memory_format=torch.channels_last)) for x in xs]
            bare = [(o[0] if isinstance(o, tuple) else o).cpu().numpy() for o in bare]
        net.train()
        D_before = [m.D for m in net.modules() if hasattr(m, "alterD")]
        before = _state_bits(net)
        ev = EvalStep(net, channels_last=True, qconv=True)
        with ev:
            assert not net.training
            eager = [ev(x, y).clone() for x, y in zip(xs, ys)]
            res_eager, cnt_eager = ev.result(), ev.counts()
        assert net.training and all(m.training for m in net.modules())
        assert _same_state(before, _state_bits(net))
        assert all(a is b for a, b in zip(D_before, [m.D for m in net.modules() if hasattr(m, "alterD")]))     # ADMM.D untouched
        for a, b in zip(eager, bare):
            a, b = a.cpu().numpy().ravel(), b.ravel()
            cos = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
            print("EvalStep vs model.eval(): cos %.7f, median |d| %.3e, max |d| %.3e" % (cos, np.median(np.abs(a - b)), np.abs(a - b).max()))
            assert cos > 0.9995, cos
            assert np.median(np.abs(a - b)) < 2e-3 * max(1.0, float(np.abs(b).max()))
        exp = [metrics_numpy(l.cpu().numpy(), y.cpu().numpy()) for l, y in zip(eager, ys)]
        assert list(cnt_eager[1:]) == [sum(e[i] for e in exp) for i in (1, 2, 3)]
        np.testing.assert_allclose(cnt_eager[0], sum(e[0] for e in exp), rtol=2e-6)
        assert res_eager[3] == 340 and abs(res_eager[1] - 100.0 * cnt_eager[1] / 340) < 1e-9
        # captured: the same bits, the short batch eagerly, the same accumulator
        with ev:
            ev.capture(xs[0], ys[0], warmup=2)
            assert ev.counts()[3] == 0                                 # the warm-up batches do not count
            cap = [ev(x, y).clone() for x, y in zip(xs, ys)]
            assert ev._graph is not None
            cnt_cap = ev.counts()
        for a, b in zip(cap, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert np.array_equal(np.array(cnt_cap[1:]), np.array(cnt_eager[1:])) and cnt_cap[0] == cnt_eager[0]
        assert _same_state(before, _state_bits(net))
        # a second evaluation through the same graph (filters re-quantised in place)
        with ev:
            again = [ev(x, y).clone() for x, y in zip(xs[:2], ys[:2])]
        for a, b in zip(again, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size = 128


def test_training_step_after_evaluation_gives_the_same_bits(dev):
    from alignq_amd import config
    from alignq_amd.eval_step import EvalStep
    try:
        outs = []
        for with_eval in (False, True):
            net, step = _cifar_net(dev, "admm", [1, 1, 1], 4, 21)
            g = torch.Generator(device="cpu").manual_seed(9)
            x, y = torch.randn(128, 3, 32, 32, generator=g).to(dev), torch.randint(0, 10, (128,), generator=g).to(dev)
            if with_eval:
                with EvalStep(net, channels_last=True, qconv=True) as ev:
                    ev(x[:100].contiguous(), y[:100].contiguous())
                    ev(x[:28].contiguous(), y[:28].contiguous())
                    assert ev.result()[3] == 128
            logits, ce, tl = step(x, y)
            outs.append((logits.clone(), ce.clone(), tl.clone(), _state_bits(net)))
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
        assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
        assert _same_state(outs[0][3], outs[1][3])
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size = 128


@pytest.mark.parametrize("kind", ["dann", "dsan"])
def test_eval_step_resnet50_batch28_capture_and_state(dev, kind):
    """ResNet-50 (DANN class logits / DSAN s_pred) at batch 28: captured replay equals the eager EvalStep bit for bit, a short
    batch runs eagerly, state_dict untouched, and the logits agree with the `model.eval()` forward being replaced."""
    from alignq_amd import config
    from alignq_amd.eval_step import EvalStep
    from alignq_amd.resnet_office import resnet50_dann, resnet50_dsan
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 28
    try:
        torch.manual_seed(31)
        net = (resnet50_dann if kind == "dann" else resnet50_dsan)(8, 8).to(dev).to(memory_format=torch.channels_last)
        net.train()
        for m in net.modules():          # the same convolution kernels in both paths (OfficeTrainStep(qconv=True) sets this)
            if hasattr(m, "quantize_fn"):
                m.use_qconv = True
        with torch.no_grad():            # running statistics away from (0, 1)
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0.0, 0.2)
                    m.running_var.uniform_(0.5, 1.5)
        g = torch.Generator(device="cpu").manual_seed(4)
        xs = [torch.randn(28, 3, 224, 224, generator=g).to(dev), torch.randn(10, 3, 224, 224, generator=g).to(dev)]
        ys = [torch.randint(0, 31, (x.shape[0],), generator=g).to(dev) for x in xs]
        net.eval()
        with torch.no_grad():
            xcl = xs[0].contiguous(memory_format=torch.channels_last)
            bare = (net(xcl, 0.0)[0] if kind == "dann" else net(xcl, None, None)[0]).cpu().numpy().ravel()
        net.train()
        before = _state_bits(net)
        ev = EvalStep(net, channels_last=True, qconv=True)
        with ev:
            eager = [ev(x, y).clone() for x, y in zip(xs, ys)]
            cnt_eager = ev.counts()
        assert _same_state(before, _state_bits(net)) and net.training
        a = eager[0].cpu().numpy().ravel()
        assert np.isfinite(a).all()
        cos = float(np.dot(a, bare) / (np.linalg.norm(a) * np.linalg.norm(bare)))
        print("%s EvalStep vs model.eval(): cos %.7f, max |d| %.3e of max |logit| %.3e" % (kind, cos, np.abs(a - bare).max(), np.abs(bare).max()))
        assert cos > 0.9995, cos
        with ev:
            ev.capture(xs[0], ys[0], warmup=1)
            cap = [ev(x, y).clone() for x, y in zip(xs, ys)]
            cnt_cap = ev.counts()
        for c, e in zip(cap, eager):
            assert torch.equal(c.view(torch.int32), e.view(torch.int32))
        assert cnt_cap == cnt_eager and cnt_cap[3] == 38
        assert _same_state(before, _state_bits(net))
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size = 128


# ------------------------------------------------------------------------------------------------ against the reference
TREE_FORMULA = {"admm": ADMM, "cdf": CDF, "office": ADMM}


@pytest.mark.parametrize("tree", ["admm", "cdf", "office"])
def test_bnq_eval_kernel_against_reference_site_g17(dev, tree):
    """The kernel on fixture G17's site (the reference's relu(act_q(bn.eval()(z)) + residual), tests/golden/gen_goldens_eval.py):
    no element more than one level from the reference's, at most max(4 n_flip_ref, 8) elements one level off (n_flip_ref: how many
    levels the reference's own fp32 evaluation moves against fp64; the factor 4 because the kernel's a z + b rounds differently
    from both), and the full chain's output equal to the reference's wherever the level agrees."""
    g = load_golden("g17_eval_site_" + tree)
    r = float(g["act_range"])
    z, res, gamma, beta, mean, var = E.site_inputs(tree)
    B, C, H, W = z.shape
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()                    # noqa: E731  (channels-last memory order)
    z_t, res_t = nhwc(z).to(dev), nhwc(res).to(dev)
    vecs = tuple(t.to(dev) for t in (gamma, beta, mean, var))
    for k in (2, 4, 8):
        n_flip_ref = int(g[f"n_flip_ref_k{k}"])
        rc, xq, _ = launch(dev, z_t, C, vecs, k, r, TREE_FORMULA[tree], False, None, 0)
        assert rc == 0
        xq = xq.cpu().permute(0, 3, 1, 2).numpy()
        d = np.abs(E.levels(xq, k, r, tree) - E.levels(g[f"xq_k{k}"], k, r, tree))
        print("G17 %s k=%d: %d of %d elements one level off (n_flip_ref %d), max %d" % (tree, k, int((d == 1).sum()), d.size, n_flip_ref, int(d.max())))
        assert d.max() <= 1
        assert int((d == 1).sum()) <= max(4 * n_flip_ref, 8)
        rc, y, _ = launch(dev, z_t, C, vecs, k, r, TREE_FORMULA[tree], True, res_t, 0)
        assert rc == 0
        y = y.cpu().permute(0, 3, 1, 2).numpy()
        same = d == 0
        np.testing.assert_allclose(y[same], g[f"y_k{k}"][same], atol=1e-6, rtol=0)
        assert np.abs(y - g[f"y_k{k}"]).max() <= 2.0 * r / (2 ** k - 1) + 1e-6      # one level at most, in value


def _g18_model(tree, g, dev):
    """this repository's model for fixture G18: det_init parameters, the fixture's batch-norm buffers, channels-last, Conv2d_Q on the
    repository's kernels (what TrainStep / OfficeTrainStep(channels_last=True, qconv=True) leave behind)"""
    from det_init import det_init_
    bits_ = int(g["bits"])
    if tree == "office":
        from alignq_amd.resnet_office import DANN, Bottleneck, ResNet
        net = DANN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), bits_, bits_, str(g["stage"]))
    else:
        from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
        net = PreActResNet(PreActBlock_conv_Q, [1, 1, 1], bits_, bits_, "second", 10, tree=tree)
    assert [n for n, _ in net.named_parameters()] == list(g["names"])
    det_init_(net)
    bufs = dict(net.named_buffers())
    keys = [k for k in g if k.startswith("buf/")]
    assert keys and all(k[4:] in bufs for k in keys)
    with torch.no_grad():
        for k in keys:
            bufs[k[4:]].copy_(torch.from_numpy(g[k]))
    net = net.to(dev).to(memory_format=torch.channels_last)
    for m in net.modules():
        if hasattr(m, "quantize_fn"):
            m.use_qconv = True
    return net.train()


@pytest.mark.parametrize("tree", ["admm", "cdf", "office"])
def test_eval_step_against_reference_network_g18(dev, tree):
    """EvalStep on fixture G18 (the reference's eval-mode network after training-mode forwards; logits, cross-entropy and
    utils.accuracy's Prec@1 / Prec@5): the precision counts equal the reference's, and the logits are no further from the
    reference's than twice the error of the `model.eval()` forward that EvalStep replaces (same weights, layout and use_qconv,
    measured here; floor 1e-5).  The yardstick is the path being replaced; the factor 2 because bin flips are discrete events."""
    from alignq_amd import config
    from alignq_amd.eval_step import EvalStep
    g = load_golden("g18_eval_net_" + tree)
    B = int(g["batch"])
    config.args.bitW = config.args.abitW = int(g["bits"])
    config.args.train_batch_size = config.args.eval_batch_size = B
    config.args.act_range = float(g["act_range"])
    try:
        net = _g18_model(tree, g, dev)
        _, xev, y = E.net_inputs(tree, int(g["target_seed"]))
        x = xev.to(dev).contiguous(memory_format=torch.channels_last)
        y = y.to(dev)
        net.eval()
        with torch.no_grad():
            out = net(x, 0.0)[0] if tree == "office" else net(x)
            parent = (out[0] if isinstance(out, tuple) else out).cpu().numpy()
        net.train()
        with EvalStep(net, channels_last=True, qconv=True) as ev:
            logits = ev(x, y).cpu().numpy()
            ce, prec1, prec5, n = ev.result()
        ref = g["logits"]
        err_parent, err_new = float(np.abs(parent - ref).max()), float(np.abs(logits - ref).max())
        print("G18 %s: max |logits - reference| EvalStep %.3e, model.eval() %.3e (max |logit| %.3e); ce %.6f (reference %.6f); "
              "Prec@1 %.4f (%.4f) Prec@5 %.4f (%.4f)" % (tree, err_new, err_parent, float(np.abs(ref).max()), ce, float(g["ce"]),
                                                         prec1, float(g["prec1"]), prec5, float(g["prec5"])))
        assert n == B
        assert round(prec1 * B / 100.0) == round(float(g["prec1"]) * B / 100.0)
        assert round(prec5 * B / 100.0) == round(float(g["prec5"]) * B / 100.0)
        assert err_new <= max(2.0 * err_parent, 1e-5)
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100
        config.args.act_range = 2.0
