"""DenseNet's evaluation without concatenations on the GPU (include/alignq_dense.h, csrc/dense_eval_kernels.hip, alignq_amd/fused.py
dense_layer_eval / avgpool2_into, alignq_amd/densenet.py DenseNet._forward_eval inside EvalStep).

Kernels: bit for bit against the launches they replace (alignq_site_eval_fwd into a contiguous temporary, then alignq_k3conv_fwd) and
against the NumPy statement of the pool, every output in a sentinel-filled window between guards, every launch twice (same bits);
the fp64 oracle of tests/dense_eval_oracle.py at the bar of tests/test_gpu_k3conv.py.  Network: depth 10 (two layers per block)
against a twin built here from the replaced launches, the launch counts, captured replay, packed weights, the flag off, the
fall-backs, and fixture G22 (the reference's eval-mode DenseNet).

Measured on MI355X (the G22 test prints them): max |logits - reference| of the fused path and of this repository's model.eval()
forward - see NOTES.md, "DenseNet-40 evaluation"."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dense_eval_oracle as DO
from tests.conftest import load_golden
from tests.golden.densenet_init import REDUCED, densenet_init_
from tests.test_gpu_k3conv import bar, count_calls
from tests.test_gpu_mobile_eval import SENTINEL, Arena, bare_eval, same_state, state_bits

pytestmark = pytest.mark.gpu

R = 2.0
CL = torch.channels_last
NAN_FILL = 0x7FC01234          # the quiet NaN the channels behind CIN hold before a launch (not the guards' sentinel)
F = torch.nn.functional


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def range2():
    from alignq_amd import config
    old = config.args.act_range
    config.args.act_range = R
    yield
    config.args.act_range = old


def dev_vec(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ------------------------------------------------------------------------------------------------ (a) one dense layer
def replaced_launches(x_t, vecs_t, eps, bins, c, dev):
    """alignq_site_eval_fwd into a contiguous temporary, then alignq_k3conv_fwd: (y [P, COUT], the temporary [P, CIN])"""
    from alignq_amd import _lib as L
    lib = L.load()
    B, H, W = c["grid"]
    P, cin, cout = B * H * W, c["cin"], c["cout"]
    g, b, m, v = vecs_t
    tmp = torch.empty(P * cin, dtype=torch.float32, device=dev)
    rec = L.EvalSite(L.ptr(x_t), L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), eps, c["k"], c["clamp"])
    assert lib.alignq_site_eval_fwd(ctypes.byref(rec), P, cin, R, c["formula"], None, L.ptr(tmp), L.stream_ptr()) == 0
    y = torch.empty(P * cout, dtype=torch.float32, device=dev)
    assert lib.alignq_k3conv_fwd(L.ptr(tmp), L.ptr(bins), L.ptr(y), B, H, W, cin, cout, c["w_bit"], L.stream_ptr()) == 0
    torch.cuda.synchronize()
    return y.view(P, cout), tmp.view(P, cin)


def fused_launch(x_ptr, ldx, y_ptr, ldy, vecs_t, eps, bins, c):
    from alignq_amd import _lib as L
    B, H, W = c["grid"]
    g, b, m, v = vecs_t
    rec = L.DenseSite(L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), eps, c["k"], c["clamp"])
    rc = L.load().alignq_dense_layer_eval_fwd(x_ptr, ldx, y_ptr, ldy, ctypes.byref(rec), L.ptr(bins), B, H, W, c["cin"], c["cout"],
                                              c["w_bit"], R, c["formula"], L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run_case(c, dev):
    """one row of the table: the fused launch twice in guarded windows; returns (y bits [P, COUT] int32, reference y, temporary, wq)"""
    from alignq_amd import ops
    B, H, W = c["grid"]
    P, cin, cout = B * H * W, c["cin"], c["cout"]
    x, vecs, eps, wq = DO.operands(c)
    x_t = torch.from_numpy(x.reshape(P, cin)).to(dev)
    vecs_t = tuple(dev_vec(a, dev) for a in vecs)
    wq_t = torch.from_numpy(wq).to(dev).contiguous(memory_format=CL)
    bins = ops.pack_filter_bins([wq_t], c["w_bit"])[0][0]
    want, tmp = replaced_launches(x_t.reshape(-1), vecs_t, eps, bins, c, dev)
    ldx, ldy, off = DO.pitches(c)
    outs = []
    if off is None:
        arena = Arena(dev, P * cout)
        for _ in range(2):
            arena.reset()
            assert fused_launch(x_t.data_ptr(), ldx, arena.view.data_ptr(), ldy, vecs_t, eps, bins, c) == 0, c["id"]
            outs.append(arena.take().view(P, cout))
    else:
        arena = Arena(dev, P * ldx)
        window = arena.view.view(torch.int32).view(P, ldx)
        for _ in range(2):
            arena.reset()
            window[:, :cin] = x_t.view(torch.int32)
            window[:, cin:] = NAN_FILL                         # everything behind the input is NaN before the launch
            base = arena.view.data_ptr()
            assert fused_launch(base, ldx, base + 4 * cin, ldy, vecs_t, eps, bins, c) == 0, c["id"]
            got = arena.take().view(P, ldx)
            assert torch.equal(got[:, :cin], x_t.view(torch.int32)), c["id"]                      # the input is only read
            assert bool((got[:, cin + cout:] == NAN_FILL).all()), c["id"]                         # the spare channels keep their bits
            outs.append(got[:, cin:cin + cout].contiguous())
    assert torch.equal(outs[0], outs[1]), ("two launches on the same inputs gave different bits", c["id"])
    assert not bool((outs[0] == SENTINEL).any()) and not bool((outs[0] == NAN_FILL).any()), ("part of the output was not written", c["id"])
    return outs[0], want, tmp, wq_t, (x, vecs, eps, wq)


@pytest.mark.parametrize("cin,cout", DO.CHANNELS, ids=["%dto%d" % s for s in DO.CHANNELS])
def test_layer_equals_site_then_convolution_and_oracle(dev, cin, cout):
    """every grid and pitch of the table at one channel pair: the bits of alignq_site_eval_fwd -> alignq_k3conv_fwd, finite outputs
    with NaN behind the input, and the fp64 oracle at test_gpu_k3conv.py's bar"""
    mine = [c for c in DO.CASES if (c["cin"], c["cout"]) == (cin, cout)]
    assert len(mine) >= len(DO.GRIDS) * len(DO.PITCHES)
    for c in mine:
        B, H, W = c["grid"]
        got_bits, want, tmp, wq_t, (x, vecs, eps, wq) = run_case(c, dev)
        got = got_bits.view(torch.float32)
        assert bool(torch.isfinite(got).all()), c["id"]
        assert torch.equal(got_bits, want.view(torch.int32)), (c["id"], float((got - want).abs().max()))
        # the oracle's site is the temporary's bits (so unzeroed padding would show in both comparisons), its fp64 convolution the bar
        s = DO.site(x, vecs, eps, c["k"], R, c["formula"], c["clamp"])
        assert np.array_equal(s.reshape(-1).view(np.uint32), tmp.cpu().numpy().reshape(-1).view(np.uint32)), c["id"]
        ref64 = torch.from_numpy(DO.conv3x3_f64(s, wq).reshape(B * H * W, cout))
        t32 = F.conv2d(tmp.view(B, H, W, cin).permute(0, 3, 1, 2), wq_t, None, 1, 1).permute(0, 2, 3, 1).reshape(B * H * W, cout)
        bar(got.cpu(), ref64, t32.cpu(), c["id"])


def test_refusals_leave_the_buffer_untouched(dev):
    c = dict(DO.CASES[3])
    x, vecs, eps, wq = DO.operands(c)
    from alignq_amd import _lib as L
    from alignq_amd import ops
    B, H, W = c["grid"]
    P, cin, cout = B * H * W, c["cin"], c["cout"]
    vecs_t = tuple(dev_vec(a, dev) for a in vecs)
    bins = ops.pack_filter_bins([torch.from_numpy(wq).to(dev).contiguous(memory_format=CL)], c["w_bit"])[0][0]
    arena = Arena(dev, P * (cin + cout))
    base = arena.view.data_ptr()
    ld = cin + cout
    for what, kw in (("ldx below CIN", dict(ldx=cin - 4)), ("ldy no multiple of 4", dict(ldy=ld + 2)), ("misaligned y", dict(y=base + 4 * cin + 4))):
        args = dict(x=base, ldx=ld, y=base + 4 * cin, ldy=ld)
        args.update(kw)
        assert fused_launch(args["x"], args["ldx"], args["y"], args["ldy"], vecs_t, eps, bins, c) == L.EINVAL, what
        assert arena.untouched(), what
    for bad in (dict(k=0), dict(w_bit=9), dict(formula=3), dict(clamp=5)):
        assert fused_launch(base, ld, base + 4 * cin, ld, vecs_t, eps, bins, dict(c, **bad)) == L.EINVAL, bad
        assert arena.untouched(), bad
    assert fused_launch(base, ld, base + 4 * cin, ld, vecs_t, eps, bins, dict(c, grid=(0, H, W))) == L.EUNSUPPORTED and arena.untouched()


# ------------------------------------------------------------------------------------------------ (b) the pool
@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
@pytest.mark.parametrize("shape", DO.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_bit_identical_to_statement_and_close_to_torch(dev, shape, pitched):
    from alignq_amd import _lib as L
    B, H, W, C = shape
    Ho, Wo = H // 2, W // 2
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    x_t = torch.from_numpy(x).to(dev)
    ld = C + 12 if pitched else C
    Po = B * Ho * Wo
    arena = Arena(dev, Po * ld)
    outs = []
    for _ in range(2):
        arena.reset()
        rc = L.load().alignq_avgpool2_nhwc_fwd(L.ptr(x_t), arena.view.data_ptr(), ld, B, H, W, C, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        got = arena.take().view(Po, ld)
        assert bool((got[:, C:] == SENTINEL).all())                      # nothing behind the C channels of a pixel is written
        outs.append(got[:, :C].contiguous())
    assert torch.equal(outs[0], outs[1]) and not bool((outs[0] == SENTINEL).any())
    want = DO.pool(x).reshape(Po, C)
    got = outs[0].cpu().numpy().view(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # F.avg_pool2d: a four-term fp32 sum in any order, 3 * 2^-24 of the window's mean |x|
    t = F.avg_pool2d(x_t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(Po, C).cpu().numpy()
    mean_abs = np.abs(x[:, :2 * Ho, :2 * Wo].astype(np.float64)).reshape(B, Ho, 2, Wo, 2, C).mean(axis=(2, 4)).reshape(Po, C)
    d = np.abs(got.astype(np.float64) - t.astype(np.float64))
    print("pool %s: max |d| / (mean |x|) = %.3e (bound %.3e)" % (shape, float((d / mean_abs).max()), 3 * 2.0 ** -24))
    assert (d <= 3 * 2.0 ** -24 * mean_abs).all()


# ------------------------------------------------------------------------------------------------ (c) the network, depth 10
def move_statistics(net, buffers=None):
    g = torch.Generator().manual_seed(78)
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                if buffers is None:
                    m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                    m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                else:
                    for b in ("running_mean", "running_var", "num_batches_tracked"):
                        getattr(m, b).copy_(torch.from_numpy(np.asarray(buffers[f"buf_{name}.{b}"])))


def reduced_net(dev, bits=4, abits=None, stage="no_align", buffers=None, dense_eval=True):
    from alignq_amd import densenet as D
    net = densenet_init_(D.DenseNet(bits, bits if abits is None else abits, stage, **REDUCED))
    move_statistics(net, buffers)
    return D.use_hip_convs(net.to(dev), dense_eval=dense_eval).train()


def batch(dev, seed, B=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


NEW = ("alignq_dense_layer_eval_fwd", "alignq_avgpool2_nhwc_fwd")


def twin_logits(net, x):
    """the forward from the launches the fused path replaces, on the filters EvalStep parked: site_eval_any, alignq_k3conv_fwd,
    torch.cat, alignq_pwconv_fwd, the new pool into a contiguous tensor"""
    from alignq_amd import _lib as L
    from alignq_amd import fused
    lib = L.load()
    x = x.contiguous(memory_format=CL)
    with torch.no_grad():
        h = net.conv1(x)
        for dense, trans in ((net.dense1, net.trans1), (net.dense2, net.trans2), (net.dense3, None)):
            for layer in dense:
                s = fused.site_eval_any(layer.bn1, layer.act_q0, h, fused.CLAMP_RELU)
                assert s is not None
                conv = layer.conv1
                rec = conv.quantize_fn.parked
                B, cin, H, W = s.shape
                y = torch.empty((B, conv.out_channels, H, W), dtype=torch.float32, device=x.device, memory_format=CL)
                L.check(lib.alignq_k3conv_fwd(L.ptr(s), L.ptr(rec.bins[0]), L.ptr(y), B, H, W, cin, conv.out_channels,
                                              conv.quantize_fn.w_bit, L.stream_ptr()), "alignq_k3conv_fwd")
                h = torch.cat((h, y), 1)
                assert h.is_contiguous(memory_format=CL)
            if trans is not None:
                s = fused.site_eval_any(trans.bn1, trans.act_q0, h, fused.CLAMP_RELU)
                assert s is not None
                conv = trans.conv1
                rec = conv.quantize_fn.parked
                B, cin, H, W = s.shape
                z = torch.empty((B, conv.out_channels, H, W), dtype=torch.float32, device=x.device, memory_format=CL)
                L.check(lib.alignq_pwconv_fwd(L.ptr(s), L.ptr(rec.bins[0]), L.ptr(z), B * H * W, cin, conv.out_channels,
                                              conv.quantize_fn.w_bit, L.stream_ptr()), "alignq_pwconv_fwd")
                h = torch.empty((B, conv.out_channels, H // 2, W // 2), dtype=torch.float32, device=x.device, memory_format=CL)
                L.check(lib.alignq_avgpool2_nhwc_fwd(L.ptr(z), L.ptr(h), conv.out_channels, B, H, W, conv.out_channels, L.stream_ptr()),
                        "alignq_avgpool2_nhwc_fwd")
        s = fused.site_eval_any(net.bn, net.act_q0, h, fused.CLAMP_RELU)
        assert s is not None
        return net.fc(net.avgpool(s).reshape(s.size(0), -1))


def test_eval_step_equals_the_twin_and_counts_its_launches(dev, monkeypatch, range2):
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(dev)
    x, y = batch(dev, 31)
    calls = count_calls(monkeypatch, *NEW, "alignq_k3conv_fwd", "alignq_pwconv_fwd", "alignq_site_eval_fwd")
    cats = []
    cat = torch.cat
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        assert all(layer.conv1.quantize_fn.parked is not None and layer.conv1.quantize_fn.parked.bins is not None
                   for dense in (net.dense1, net.dense2, net.dense3) for layer in dense)
        with monkeypatch.context() as mp:
            mp.setattr(torch, "cat", lambda *a, **kw: (cats.append(1), cat(*a, **kw))[1])
            logits = ev(x, y).clone()
        # six dense layers one launch each, two pitched pools, no stand-alone 3x3 convolution, no concatenation; the sites that are
        # left are the two transitions' and the head's
        assert calls == {"alignq_dense_layer_eval_fwd": 6, "alignq_avgpool2_nhwc_fwd": 2, "alignq_k3conv_fwd": 0, "alignq_pwconv_fwd": 2,
                         "alignq_site_eval_fwd": 3}, calls
        assert cats == []
        twin = twin_logits(net, x)
        assert calls["alignq_k3conv_fwd"] == 6
    assert torch.isfinite(logits).all() and tuple(logits.shape) == (8, 10)
    assert torch.equal(logits.view(torch.int32), twin.view(torch.int32)), float((logits - twin).abs().max())


def test_captured_replay_state_and_flags(dev, range2):
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(dev)
    batches = [batch(dev, 40 + i) for i in range(2)]
    before = state_bits(net)
    assert net.fuse_dense_eval is True
    ev = EvalStep(net, channels_last=True, qconv=True)
    with ev:
        assert not net.training
        eager = [ev(x, y).clone() for x, y in batches]
        acc_eager = ev._acc.clone()
    assert net.training and all(m.training for m in net.modules())
    assert same_state(before, state_bits(net))
    with ev:
        ev.capture(*batches[0], warmup=2)
        assert ev.counts()[3] == 0
        cap = [ev(x, y).clone() for x, y in batches]
        assert ev._graph is not None
        acc_cap = ev._acc.clone()
    for a, b in zip(cap, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(acc_cap, acc_eager)
    assert same_state(before, state_bits(net)) and net.fuse_dense_eval is True
    assert all(c.quantize_fn.parked is None for c in ev.all_convs)


def test_running_statistics_may_change_under_a_captured_graph(dev, range2):
    """the coefficients are formed inside the launch: after the running statistics change in place, a replay equals a fresh eager run"""
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(dev)
    x, y = batch(dev, 50)
    ev = EvalStep(net, channels_last=True, qconv=True)
    with ev:
        ev.capture(x, y, warmup=1)
        first = ev(x, y).clone()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.add_(0.05)
                    m.running_var.mul_(1.25)
        replay = ev(x, y).clone()
    with EvalStep(net, channels_last=True, qconv=True) as ev2:
        eager = ev2(x, y).clone()
    assert not torch.equal(first, replay)
    assert torch.equal(replay.view(torch.int32), eager.view(torch.int32))


def test_packed_weights_give_the_same_logits(dev, range2):
    from alignq_amd import densenet as D
    from alignq_amd import export
    from alignq_amd.eval_step import EvalStep
    net = reduced_net(dev)
    pk = export.pack_model(net)
    skeleton = D.use_hip_convs(D.DenseNet(4, 4, "no_align", **REDUCED).to(dev), dense_eval=True)
    pk.apply(skeleton)
    with torch.no_grad():
        for name, c in export.quantised_convs(skeleton):
            c.weight.fill_(float("nan"))                               # the fp32 filters are never read
    x, y = batch(dev, 60)
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        want, cnt = ev(x, y).clone(), ev.counts()
    with EvalStep(skeleton, weights=pk) as ev2:
        got, cnt2 = ev2(x, y).clone(), ev2.counts()
    assert torch.isfinite(want).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and cnt == cnt2


def test_flag_off_runs_todays_launches(dev, monkeypatch, range2):
    """without the flag EvalStep on a DenseNet is the composition: none of the new entry points, six stand-alone 3x3 convolutions and
    six concatenations, and the logits of a model that never carried the flag"""
    from alignq_amd.eval_step import EvalStep
    never = reduced_net(dev, dense_eval=False)
    assert never.fuse_dense_eval is False and "fuse_dense_eval" not in never.__dict__
    x, y = batch(dev, 70)
    with EvalStep(never, channels_last=True, qconv=True) as ev:
        want = ev(x, y).clone()
    net = reduced_net(dev)
    net.fuse_dense_eval = False
    calls = count_calls(monkeypatch, *NEW, "alignq_k3conv_fwd")
    cats = []
    cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **kw: (cats.append(1), cat(*a, **kw))[1])
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        got = ev(x, y).clone()
    assert calls == {"alignq_dense_layer_eval_fwd": 0, "alignq_avgpool2_nhwc_fwd": 0, "alignq_k3conv_fwd": 6} and len(cats) == 6
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # and a bare model.eval() forward never takes the fused path, flag or not
    net.fuse_dense_eval = True
    bare_eval(net, x.contiguous(memory_format=CL))
    assert calls["alignq_dense_layer_eval_fwd"] == 0 and calls["alignq_avgpool2_nhwc_fwd"] == 0


def test_fall_backs_run_the_composition(dev, monkeypatch, range2):
    """an NCHW evaluation, and a_bit == 32 in stage 'align' (the quantiser returns its transform: no folded form): the composition
    runs, no dense layer is fused, and the results are finite"""
    from alignq_amd.eval_step import EvalStep
    calls = count_calls(monkeypatch, "alignq_dense_layer_eval_fwd")
    x, y = batch(dev, 80)
    net = reduced_net(dev)
    with EvalStep(net, channels_last=False, qconv=True) as ev:
        assert x.is_contiguous() and not x.is_contiguous(memory_format=CL)
        a = ev(x, y).clone()
    assert calls["alignq_dense_layer_eval_fwd"] == 0 and torch.isfinite(a).all()
    net = reduced_net(dev, bits=4, abits=32, stage="align")
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        b = ev(x, y).clone()
    assert calls["alignq_dense_layer_eval_fwd"] == 0 and torch.isfinite(b).all()


# ------------------------------------------------------------------------------------------------ (d) the reference, fixture G22
def test_g22_targets_keep_their_margin():
    g = load_golden("g22_densenet_eval")
    lg, y = g["logits"], g["targets"]
    order = np.argsort(-lg, axis=1)
    span = lg.max(axis=1) - lg.min(axis=1)
    for i, t in enumerate(y):
        others = [lg[i, order[i, b]] for b in (0, 1, 4, 5) if order[i, b] != t]
        assert min(abs(lg[i, t] - o) for o in others) >= float(g["margin_fraction"]) * span[i]
    assert float(g["margin_fraction"]) == 0.05 and float(g["min_margin"]) > 0.1
    assert int(g["bits"]) == 8 and int(g["depth"]) == 10 and int(g["batch"]) == 8 and tuple(g["x"].shape) == (8, 3, 32, 32)
    assert 0 < int(g["n_top1"]) < int(g["n_top5"]) < int(g["batch"])


def test_eval_step_against_reference_network_g22(dev, range2):
    """EvalStep with the fused dense layers on fixture G22 (the reference's eval-mode DenseNet, depth 10, 8W/8A, after three
    training-mode forwards): the precision counts equal the reference's, and the logits are no further from the reference's than twice
    the error of this repository's existing `model.eval()` forward on the same inputs (the parent's path, not the code under test)."""
    from alignq_amd.eval_step import EvalStep
    g = load_golden("g22_densenet_eval")
    B, bits = int(g["batch"]), int(g["bits"])
    assert float(g["act_range"]) == R
    net = reduced_net(dev, bits=bits, stage=str(g["stage"]), buffers=g)
    x = torch.from_numpy(g["x"]).to(dev).contiguous(memory_format=CL)
    y = torch.from_numpy(g["targets"]).to(dev)
    parent = bare_eval(net, x).cpu().numpy()
    with EvalStep(net, channels_last=True, qconv=True) as ev:
        logits = ev(x, y).cpu().numpy()
        ce_sum, n1, n5, n = ev.counts()
    ref, min_margin = g["logits"], float(g["min_margin"])
    err_parent, err_new = float(np.abs(parent - ref).max()), float(np.abs(logits - ref).max())
    print("G22: max |logits - reference| fused EvalStep %.3e, model.eval() %.3e (max |logit| %.3e, min_margin %.3e); ce %.6f "
          "(reference %.6f); top-1 %d (%d) top-5 %d (%d)" % (err_new, err_parent, float(np.abs(ref).max()), min_margin, ce_sum / n,
                                                           float(g["ce"]), n1, int(g["n_top1"]), n5, int(g["n_top5"])))
    assert 2.0 * err_new < min_margin, "fixture problem: G22's targets are not far enough from the rank boundaries for this error"
    assert (n1, n5, n) == (int(g["n_top1"]), int(g["n_top5"]), B)
    assert err_new <= 2.0 * err_parent
