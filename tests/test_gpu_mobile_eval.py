"""MobileNet-V2's folded evaluation sites on the GPU (include/alignq_mobile.h, csrc/mobile_eval_kernels.hip, alignq_amd/fused.py
site_eval_any / site_eval_twin / dw_site_eval, alignq_amd/mobilenet.py inside EvalStep).

Kernels: bit for bit against tests/mobile_eval_oracle.py and against the launches they replace, every output written into a
sentinel-filled window between guards, every launch twice (same bits).  Model: fixture G20 (the reference's test() forward), the
routing of every site, captured replay, packed weights, one full-size batch."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import mobile_eval_oracle as MO
from tests.conftest import load_golden
from tests.golden.mobilenet_init import REDUCED_CFG, mobilenet_init_

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC05A5A         # a quiet NaN no kernel here produces
GUARD = 64
R = 2.0
EPS = 1e-5
ADMM, CDF = MO.ADMM, MO.CDF
NONE, RELU, RELU6 = MO.NONE, MO.RELU, MO.RELU6
CL = torch.channels_last

# the site kernels run at most 2048 workgroups of 4 x 256 float4 per pass: one pass covers 2,097,152 float4.  (1, 20, 648, 648) has
# 419,904 pixels x 5 quads = 2,099,520 float4: a second grid-stride pass of 2,368 float4 whose quads start (2^21 mod 5 = 2) off the first's
MULTI_PASS = (1, 20, 648, 648)
SITE_SHAPES = [(2, 4, 1, 1), (3, 20, 5, 7), (2, 144, 9, 9), (4, 960, 4, 4), (2, 1280, 4, 4), (8, 96, 32, 32), MULTI_PASS]
TWIN_SHAPES = [(3, 20, 5, 7), (2, 24, 8, 8), (2, 320, 4, 4), MULTI_PASS]
# the last one goes beyond one pass of the depthwise launch's 1024 workgroups (1152 workgroups' worth at stride 1)
DW_SHAPES = [(2, 4, 1, 1), (3, 20, 5, 7), (3, 20, 6, 8), (2, 144, 9, 9), (4, 960, 4, 4), (8, 144, 32, 32)]
DW_CASES = [(shape, s) for shape in DW_SHAPES for s in (1, 2)]
FP32_FILTER_CASE = ((3, 20, 5, 7), 2)       # the one case with an unquantised filter


def ids(shape):
    return "x".join(map(str, shape))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Arena:
    """one 16-byte aligned window of n floats in a sentinel-filled device buffer, GUARD elements on either side"""

    def __init__(self, dev, n):
        self.n, self.off = n, GUARD
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and GUARD % 4 == 0
        self.view = self.buf[GUARD:GUARD + n].view(torch.float32)

    def reset(self):
        self.buf.fill_(SENTINEL)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def take(self):
        """the window's bits (a copy on the device); asserts that the guards still hold the sentinel"""
        assert self.guards_intact(), "a kernel wrote outside its tensor"
        return self.buf[GUARD:GUARD + self.n].clone()


def dbits(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(dev).view(torch.int32)


def up(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(dev) for a in arrays]


def bn_vectors(rng, C):
    gamma = (0.5 + rng.random(C)).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
    mean = (rng.standard_normal(C) * 0.5 + 0.2).astype(np.float32)
    var = (0.3 + 2.0 * rng.random(C)).astype(np.float32)
    return gamma, beta, mean, var


def record(z_t, vecs_t, k, clamp, eps=EPS):
    from alignq_amd import _lib as L
    g, b, m, v = vecs_t
    return L.EvalSite(L.ptr(z_t), L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), eps, k, clamp)


def run_site(z_t, vecs_t, P, C, k, r, formula, clamp, res_t, y_t):
    from alignq_amd import _lib as L
    rec = record(z_t, vecs_t, k, clamp)
    rc = L.load().alignq_site_eval_fwd(ctypes.byref(rec), P, C, r, formula, L.ptr(res_t), L.ptr(y_t), L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run_twin(zA, vA, kA, zB, vB, kB, clampB, P, C, r, formula, y_t, clampA=NONE):
    from alignq_amd import _lib as L
    a, b = record(zA, vA, kA, clampA), record(zB, vB, kB, clampB)
    rc = L.load().alignq_site_eval_twin_fwd(ctypes.byref(a), ctypes.byref(b), P, C, r, formula, L.ptr(y_t), L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run_dw(x_t, w_t, vecs_t, shape, s, k, r, formula, clamp, y_t):
    from alignq_amd import _lib as L
    B, C, H, W = shape
    rec = record(None, vecs_t, k, clamp)
    rc = L.load().alignq_dwconv3x3_site_eval_fwd(L.ptr(x_t), L.ptr(w_t), ctypes.byref(rec), B, H, W, C, s, r, formula, L.ptr(y_t),
                                                 L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def twice(arena, launch):
    """the launch into a fresh arena, twice: return code 0, the guards intact, the same bits"""
    outs = []
    for _ in range(2):
        arena.reset()
        assert launch() == 0
        outs.append(arena.take())
    assert torch.equal(outs[0], outs[1]), "two launches on the same inputs gave different bits"
    assert not bool((outs[0] == SENTINEL).any()), "part of the output was not written"
    return outs[0]


# ------------------------------------------------------------------------------------------------ (a) one site
@pytest.mark.parametrize("formula", [ADMM, CDF], ids=["admm", "cdf"])
@pytest.mark.parametrize("shape", SITE_SHAPES, ids=ids)
def test_site_bit_identical_to_oracle(dev, shape, formula):
    B, C, H, W = shape
    rng = np.random.default_rng(2000 + C + B)
    z = rng.standard_normal((B, H, W, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    res = rng.standard_normal((B, H, W, C), dtype=np.float32)
    vecs = bn_vectors(rng, C)
    x = MO.affine(z, *vecs, EPS)
    z_t, res_t = up(dev, z, res)
    vecs_t = up(dev, *vecs)
    arena = Arena(dev, z.size)
    n = 0
    for k in (2, 4, 8, 32):
        xq = MO.quant(x, k, R, formula)
        for clamp, with_res in itertools.product((NONE, RELU, RELU6), (False, True)):
            got = twice(arena, lambda: run_site(z_t, vecs_t, B * H * W, C, k, R, formula, clamp, res_t if with_res else None, arena.view))
            exp = dbits(MO.finish(xq, clamp, res if with_res else None), dev)
            if not torch.equal(got, exp):
                raise AssertionError(f"{int((got != exp).sum())} of {z.size} elements differ: k={k} clamp={clamp} res={with_res}")
            n += 1
    assert n == 4 * 3 * 2


@pytest.mark.parametrize("shape", [(3, 64, 7, 5), (2, 4, 3, 3), (1, 2048, 2, 3)], ids=ids)
def test_site_equals_bnq_eval_fwd_at_power_of_two_channels(dev, shape):
    from alignq_amd import _lib as L
    lib = L.load()
    B, C, H, W = shape
    rng = np.random.default_rng(2100 + C)
    z = rng.standard_normal((B, H, W, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    res = rng.standard_normal((B, H, W, C), dtype=np.float32)
    z_t, res_t = up(dev, z, res)
    g, b, m, v = vecs_t = up(dev, *bn_vectors(rng, C))
    arena, old = Arena(dev, z.size), torch.empty(z.size, dtype=torch.float32, device=dev)
    for formula, k, relu, with_res in itertools.product((ADMM, CDF), (2, 4, 8, 32), (0, 1), (False, True)):
        rt = res_t if with_res else None
        assert lib.alignq_bnq_eval_fwd(L.ptr(z_t), B * H * W, C, L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), EPS, k, R, formula, relu,
                                       L.ptr(rt), L.ptr(old), None, 0, L.stream_ptr()) == 0
        got = twice(arena, lambda: run_site(z_t, vecs_t, B * H * W, C, k, R, formula, RELU if relu else NONE, rt, arena.view))
        assert torch.equal(got, old.view(torch.int32)), (formula, k, relu, with_res)


@pytest.mark.parametrize("formula", [ADMM, CDF], ids=["admm", "cdf"])
def test_relu6_upper_clamp_binds_at_act_range_8(dev, formula):
    """act_range = 8: quantiser levels reach 8, and the unquantised site (k = 32) is fed values beyond 6 as well"""
    B, C, H, W = shape = (3, 20, 5, 7)
    r = 8.0
    rng = np.random.default_rng(2200)
    z = rng.standard_normal((B, H, W, C), dtype=np.float32) * np.float32(6.0)
    res = rng.standard_normal((B, H, W, C), dtype=np.float32)
    vecs = bn_vectors(rng, C)
    x = MO.affine(z, *vecs, EPS)
    z_t, res_t = up(dev, z, res)
    vecs_t = up(dev, *vecs)
    arena = Arena(dev, z.size)
    for k, with_res in itertools.product((2, 4, 8, 32), (False, True)):
        xq = MO.quant(x, k, r, formula)
        pre = xq if not with_res else (xq + res).astype(np.float32)
        assert (pre > 6).sum() >= 8, (k, with_res)                       # the upper clamp really binds ...
        exp = MO.finish(xq, RELU6, res if with_res else None)
        assert exp.max() == 6.0 and ((exp > 0) & (exp < 6)).any()           # ... and not everywhere
        got = twice(arena, lambda: run_site(z_t, vecs_t, B * H * W, C, k, r, formula, RELU6, res_t if with_res else None, arena.view))
        assert torch.equal(got, dbits(exp, dev)), (k, with_res)
        assert float(arena.view.max()) == 6.0


# ------------------------------------------------------------------------------------------------ (b) the block tail
@pytest.mark.parametrize("kpair", [(4, 4), (8, 32)], ids=["k4-4", "k8-32"])
@pytest.mark.parametrize("shape", TWIN_SHAPES, ids=ids)
def test_twin_equals_two_site_launches_and_oracle(dev, shape, kpair):
    B, C, H, W = shape
    P = B * H * W
    kA, kB = kpair
    rng = np.random.default_rng(2300 + C + kA)
    zA = rng.standard_normal((B, H, W, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    zB = rng.standard_normal((B, H, W, C), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    vA, vB = bn_vectors(rng, C), bn_vectors(rng, C)
    zA_t, zB_t = up(dev, zA, zB)
    vA_t, vB_t = up(dev, *vA), up(dev, *vB)
    arena, tmp, two = Arena(dev, zA.size), Arena(dev, zA.size), Arena(dev, zA.size)
    for formula, clampB in itertools.product((ADMM, CDF), (RELU, NONE, RELU6)):
        got = twice(arena, lambda: run_twin(zA_t, vA_t, kA, zB_t, vB_t, kB, clampB, P, C, R, formula, arena.view))
        # two launches of the one-site kernel: B into a temporary, then A with the temporary as its residual
        tmp.reset(), two.reset()
        assert run_site(zB_t, vB_t, P, C, kB, R, formula, clampB, None, tmp.view) == 0
        assert run_site(zA_t, vA_t, P, C, kA, R, formula, NONE, tmp.view, two.view) == 0
        assert torch.equal(got, two.take()), (formula, clampB, "two launches")
        if clampB == RELU or zA.size < (1 << 20):
            exp = MO.twin(zA, vA, EPS, kA, zB, vB, EPS, kB, clampB, R, formula)
            assert torch.equal(got, dbits(exp, dev)), (formula, clampB, "oracle")


# ------------------------------------------------------------------------------------------------ (c) depthwise + site
def levels_relu(rng, shape):
    """what the layers really see: relu(4-bit levels * act_range), with many exact zeros"""
    lv = (2.0 * rng.integers(0, 16, shape) / 15.0 - 1.0) * R
    return np.maximum(lv, 0.0).astype(np.float32)


@pytest.mark.parametrize("idx", range(len(DW_CASES)), ids=[f"{ids(c[0])}-s{c[1]}" for c in DW_CASES])
def test_dw_site_equals_depthwise_then_site_and_oracle(dev, idx):
    from alignq_amd import _lib as L
    lib = L.load()
    shape, s = DW_CASES[idx]
    B, C, H, W = shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    rng = np.random.default_rng(2400 + idx)
    x = levels_relu(rng, (B, H, W, C)) if idx % 2 else rng.standard_normal((B, H, W, C)).astype(np.float32)
    if (shape, s) == FP32_FILTER_CASE:
        w = (rng.standard_normal((C, 1, 3, 3)) * 0.3).astype(np.float32)
    else:
        w = (2.0 * rng.integers(0, 16, (C, 1, 3, 3)) / 15.0 - 1.0).astype(np.float32)      # W_q's 4-bit level values
    vecs = bn_vectors(rng, C)
    x_t, w_t = up(dev, x, w)
    vecs_t = up(dev, *vecs)
    n_out = B * Ho * Wo * C
    arena, mid, two = Arena(dev, n_out), Arena(dev, n_out), Arena(dev, n_out)
    conv = MO.dw(x, w, s)
    assert conv.shape == (B, Ho, Wo, C)
    xa = MO.affine(conv, *vecs, EPS)
    assert lib.alignq_dwconv3x3_nhwc_fwd(L.ptr(x_t), L.ptr(w_t), L.ptr(mid.view), B, H, W, C, s, L.stream_ptr()) == 0
    assert torch.equal(mid.take(), dbits(conv, dev))
    for formula, k in itertools.product((ADMM, CDF), (4, 8, 32)):
        xq = MO.quant(xa, k, R, formula)
        for clamp in (NONE, RELU, RELU6):
            got = twice(arena, lambda: run_dw(x_t, w_t, vecs_t, shape, s, k, R, formula, clamp, arena.view))
            two.reset()
            assert run_site(mid.view, vecs_t, B * Ho * Wo, C, k, R, formula, clamp, None, two.view) == 0
            assert torch.equal(got, two.take()), (formula, k, clamp, "depthwise launch, then site launch")
            assert torch.equal(got, dbits(MO.finish(xq, clamp), dev)), (formula, k, clamp, "oracle")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched(dev):
    from alignq_amd import _lib as L
    rng = np.random.default_rng(2500)
    n = 2052 * 4
    z_t = torch.from_numpy(rng.standard_normal(n + 8).astype(np.float32)).to(dev)
    w_t = torch.from_numpy(rng.standard_normal(2052 * 9 + 8).astype(np.float32)).to(dev)
    vecs_t = up(dev, *bn_vectors(rng, 2052))
    arena = Arena(dev, n)
    y = arena.view
    cases = [
        ("C = 6", L.EUNSUPPORTED, lambda: run_site(z_t, vecs_t, 4, 6, 4, R, CDF, RELU6, None, y)),
        ("C = 2052", L.EUNSUPPORTED, lambda: run_site(z_t, vecs_t, 4, 2052, 4, R, CDF, RELU6, None, y)),
        ("k = 0", L.EINVAL, lambda: run_site(z_t, vecs_t, 4, 8, 0, R, CDF, RELU6, None, y)),
        ("misaligned z", L.EINVAL, lambda: run_site(z_t[1:], vecs_t, 4, 8, 4, R, CDF, RELU6, None, y)),
        ("misaligned y", L.EINVAL, lambda: run_site(z_t, vecs_t, 4, 8, 4, R, CDF, RELU6, None, y[1:])),
        ("misaligned residual", L.EINVAL, lambda: run_site(z_t, vecs_t, 4, 8, 4, R, CDF, RELU6, z_t[2:], y)),
        ("twin C = 6", L.EUNSUPPORTED, lambda: run_twin(z_t, vecs_t, 4, z_t, vecs_t, 4, RELU, 4, 6, R, CDF, y)),
        ("twin C = 2052", L.EUNSUPPORTED, lambda: run_twin(z_t, vecs_t, 4, z_t, vecs_t, 4, RELU, 4, 2052, R, CDF, y)),
        ("twin k = 0", L.EINVAL, lambda: run_twin(z_t, vecs_t, 4, z_t, vecs_t, 0, RELU, 4, 8, R, CDF, y)),
        ("twin misaligned z_B", L.EINVAL, lambda: run_twin(z_t, vecs_t, 4, z_t[1:], vecs_t, 4, RELU, 4, 8, R, CDF, y)),
        ("twin clamp_A", L.EINVAL, lambda: run_twin(z_t, vecs_t, 4, z_t, vecs_t, 4, RELU, 4, 8, R, CDF, y, clampA=RELU)),
        ("dw C = 6", L.EUNSUPPORTED, lambda: run_dw(z_t, w_t, vecs_t, (1, 6, 2, 2), 1, 4, R, CDF, RELU6, y)),
        ("dw C = 2052", L.EUNSUPPORTED, lambda: run_dw(z_t, w_t, vecs_t, (1, 2052, 2, 2), 1, 4, R, CDF, RELU6, y)),
        ("dw stride 3", L.EUNSUPPORTED, lambda: run_dw(z_t, w_t, vecs_t, (1, 8, 4, 4), 3, 4, R, CDF, RELU6, y)),
        ("dw k = 0", L.EINVAL, lambda: run_dw(z_t, w_t, vecs_t, (1, 8, 4, 4), 1, 0, R, CDF, RELU6, y)),
        ("dw misaligned x", L.EINVAL, lambda: run_dw(z_t[1:], w_t, vecs_t, (1, 8, 4, 4), 1, 4, R, CDF, RELU6, y)),
        ("dw misaligned filter", L.EINVAL, lambda: run_dw(z_t, w_t[3:], vecs_t, (1, 8, 4, 4), 1, 4, R, CDF, RELU6, y)),
    ]
    for what, code, call in cases:
        assert call() == code, what
        assert arena.untouched(), what
    assert run_site(z_t, vecs_t, 4, 8, 4, R, CDF, RELU6, None, y) == 0 and not arena.untouched()      # the same call, accepted


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture
def bits4():
    from alignq_amd import config
    old = (config.args.bitW, config.args.abitW, config.args.act_range, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 4
    config.args.act_range = 2.0
    yield
    (config.args.bitW, config.args.abitW, config.args.act_range, config.args.train_batch_size, config.args.eval_batch_size) = old


def reduced_net(monkeypatch, dev, stage="no_align", buffers=None):
    """the reduced model of the fixtures with running statistics away from (0, 1): G20's, or seeded ones"""
    from alignq_amd import mobilenet as M
    monkeypatch.setattr(M.MobileNetV2, "cfg", list(REDUCED_CFG))
    net = mobilenet_init_(M.mobile_v2(4, 4, stage))
    move_statistics(net, buffers)
    return M.use_hip_convs(net.to(dev)).train()


def move_statistics(net, buffers=None):
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                if buffers is None:
                    m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                    m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                else:
                    for b in ("running_mean", "running_var", "num_batches_tracked"):
                        getattr(m, b).copy_(torch.from_numpy(np.asarray(buffers[f"buf_{name}.{b}"])))


def block_strides(cfg):
    return [s for _, _, n, stride in cfg for s in [stride] + [1] * (n - 1)]


def state_bits(net):
    from alignq_amd.paths import FLAGS
    flags = {(n, f): m.__dict__.get(f, "<absent>") for n, m in net.named_modules() for f in FLAGS}
    return ({k: v.detach().clone() for k, v in net.state_dict().items()}, {n: m.training for n, m in net.named_modules()}, flags)


def same_state(a, b):
    return (a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and a[1] == b[1] and a[2] == b[2])


def bare_eval(net, x):
    was = net.training
    net.eval()
    with torch.no_grad():
        out = net(x).clone()
    net.train(was)
    return out


def test_eval_step_against_reference_network_g20(dev, monkeypatch, bits4):
    """EvalStep on fixture G20 (the reference's eval-mode MobileNet-V2 after three training-mode forwards): the precision counts equal
    the reference's, and the logits are no further from the reference's than twice the error of this repository's `model.eval()`
    forward on the same weights and layout, measured here (floor 1e-5) - the rule of test_eval_step_against_reference_network_g18."""
    from alignq_amd.eval_step import EvalStep
    g = load_golden("g20_mobilenet_eval")
    B = int(g["batch"])
    assert int(g["bits"]) == 4 and float(g["act_range"]) == 2.0
    net = reduced_net(monkeypatch, dev, str(g["stage"]), g)
    x = torch.from_numpy(g["x"]).to(dev).contiguous(memory_format=CL)
    y = torch.from_numpy(g["targets"]).to(dev)
    parent = bare_eval(net, x).cpu().numpy()
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        logits = ev(x, y).cpu().numpy()
        ce, prec1, prec5, n = ev.result()
    ref, min_margin = g["logits"], float(g["min_margin"])
    err_parent, err_new = float(np.abs(parent - ref).max()), float(np.abs(logits - ref).max())
    print("G20: max |logits - reference| EvalStep %.3e, model.eval() %.3e (max |logit| %.3e, min_margin %.3e); ce %.6f (reference "
          "%.6f); Prec@1 %.4f (%.4f) Prec@5 %.4f (%.4f)" % (err_new, err_parent, float(np.abs(ref).max()), min_margin, ce,
                                                            float(g["ce"]), prec1, float(g["prec1"]), prec5, float(g["prec5"])))
    assert 2.0 * err_new < min_margin, "fixture problem: G20's targets are not far enough from the rank boundaries for this error"
    assert n == B
    assert round(prec1 * B / 100.0) == round(float(g["prec1"]) * B / 100.0)
    assert round(prec5 * B / 100.0) == round(float(g["prec5"]) * B / 100.0)
    assert err_new <= max(2.0 * err_parent, 1e-5)


def test_every_site_takes_the_folded_route(dev, monkeypatch, bits4):
    """Inside EvalStep no nn.BatchNorm2d.forward runs, and the three folded forms are called once per site of REDUCED_CFG."""
    from alignq_amd import fused
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(monkeypatch, dev)
    strides = block_strides(REDUCED_CFG)
    n_blocks, n_s1, n_s2 = len(strides), strides.count(1), strides.count(2)
    assert (n_blocks, n_s1, n_s2) == (4, 2, 2)
    fired = []
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.register_forward_hook(lambda mod, inp, out, name=name: fired.append(name))
    calls = {"site_eval_any": [], "site_eval_twin": [], "dw_site_eval": []}
    for fn in calls:
        orig = getattr(fused, fn)

        def counted(*a, _orig=orig, _fn=fn, **kw):
            out = _orig(*a, **kw)
            calls[_fn].append((a, out))
            return out
        monkeypatch.setattr(fused, fn, counted)
    x = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(8)).to(dev).contiguous(memory_format=CL)
    y = torch.arange(8, device=dev) % 10
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        logits = ev(x, y)
    assert torch.isfinite(logits).all()
    assert fired == [], fired
    assert all(out is not None for rec in calls.values() for _, out in rec)             # no site fell back to the composition
    # stem + every block's act_q1 + the tail of every stride-2 block + head; the depthwise site of every block; the stride-1 tails
    clamps = [a[3] for a, _ in calls["site_eval_any"]]
    assert clamps.count(fused.CLAMP_RELU) == 1 + 1 and clamps.count(fused.CLAMP_RELU6) == n_blocks
    assert clamps.count(fused.CLAMP_NONE) == n_s2
    assert len(calls["site_eval_any"]) == 1 + n_blocks + n_s2 + 1
    assert len(calls["dw_site_eval"]) == n_blocks and all(a[4] == fused.CLAMP_RELU6 for a, _ in calls["dw_site_eval"])
    assert len(calls["site_eval_twin"]) == n_s1 and all(a[6] == fused.CLAMP_RELU for a, _ in calls["site_eval_twin"])
    # outside EvalStep the same model composes the modules: every batch-norm runs, none of the three is called
    before = {k: len(v) for k, v in calls.items()}
    bare_eval(net, x)
    assert len(fired) == 3 * n_blocks + n_s1 + 2 and {k: len(v) for k, v in calls.items()} == before


def test_captured_replay_state_and_bare_forward(dev, monkeypatch, bits4):
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(monkeypatch, dev)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(8, 3, 16, 16, generator=g).to(dev) for _ in range(3)] + [torch.randn(5, 3, 16, 16, generator=g).to(dev)]
    ys = [torch.randint(0, 10, (x.shape[0],), generator=g).to(dev) for x in xs]
    xcl = xs[0].contiguous(memory_format=CL)
    bare_before = bare_eval(net, xcl)
    before = state_bits(net)
    ev = EvalStep(net, channels_last=True, qconv=True)
    with ev:
        assert not net.training
        eager = [ev(x, y).clone() for x, y in zip(xs, ys)]
        acc_eager = ev._acc.clone()
    assert net.training and all(m.training for m in net.modules())
    assert same_state(before, state_bits(net))
    with ev:
        ev.capture(xs[0], ys[0], warmup=2)
        assert ev.counts()[3] == 0                                     # the warm-up batches do not count
        cap = [ev(x, y).clone() for x, y in zip(xs, ys)]              # three replays; the short last batch runs eagerly
        assert ev._graph is not None and tuple(cap[3].shape) == (5, 10)
        acc_cap = ev._acc.clone()
        assert ev.counts()[3] == 29
    for a, b in zip(cap, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(acc_cap, acc_eager)                             # the accumulator's 32 bytes
    assert same_state(before, state_bits(net))
    assert all(c.quantize_fn.parked is None for c in ev.all_convs)
    bare_after = bare_eval(net, xcl)
    assert torch.equal(bare_before.view(torch.int32), bare_after.view(torch.int32))
    d = (eager[0] - bare_before).abs().max().item()
    print("EvalStep vs model.eval(): max |d| %.3e of max |logit| %.3e" % (d, bare_before.abs().max().item()))


def test_packed_weights_give_the_same_logits(dev, monkeypatch, bits4):
    from alignq_amd import export
    from alignq_amd import mobilenet as M
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(monkeypatch, dev)
    pk = export.pack_model(net)
    dw_names = [name + ".weight" for name, m in net.named_modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]
    assert len(dw_names) == 4 and all(n in pk.filters and pk.filters[n]["shape"][1:] == [1, 3, 3] for n in dw_names)
    skeleton = M.use_hip_convs(M.mobile_v2(4, 4, "no_align").to(dev))
    pk.apply(skeleton)
    with torch.no_grad():
        for name, c in export.quantised_convs(skeleton):
            c.weight.fill_(float("nan"))                               # the fp32 filters are never read
    x = torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(10)).to(dev)
    y = torch.arange(8, device=dev) % 10
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        want, cnt = ev(x, y).clone(), ev.counts()
    with EvalStep(skeleton, weights=pk) as ev2:
        for name, c in export.quantised_convs(skeleton):
            if c.groups > 1:
                assert c.quantize_fn.parked.q.shape == c.weight.shape and bool(torch.isfinite(c.quantize_fn.parked.q).all())
        got, cnt2 = ev2(x, y).clone(), ev2.counts()
    assert torch.isfinite(want).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and cnt == cnt2


def test_full_size_batch_equals_its_captured_replay(dev, bits4):
    from alignq_amd import mobilenet as M
    from alignq_amd.eval_step import EvalStep
    net = mobilenet_init_(M.mobile_v2(4, 4, "no_align"))
    move_statistics(net)
    net = M.use_hip_convs(net.to(dev)).train()
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(100, 3, 32, 32, generator=g).to(dev), torch.randint(0, 10, (100,), generator=g).to(dev)
    ev = EvalStep(net, channels_last=True, qconv=True)
    with ev:
        eager = ev(x, y).clone()
        acc = ev._acc.clone()
    assert tuple(eager.shape) == (100, 10) and bool(torch.isfinite(eager).all())
    with ev:
        ev.capture(x, y, warmup=1)
        cap = ev(x, y).clone()
        assert ev._graph is not None and torch.equal(ev._acc, acc)
    assert torch.equal(cap.view(torch.int32), eager.view(torch.int32))
