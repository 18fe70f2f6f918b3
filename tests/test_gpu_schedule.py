"""Device-side hyper-parameters on the MI355X (alignq_amd/schedule.py; alignq_sgd_step_multi_dev, alignq_sgd_admm_step_multi_dev and
alignq_hyper_advance of csrc/multi_tensor_kernels.hip): the `_dev` launchers against the by-value launchers bit for bit (and with
them against the float64 statement of tests/weights_oracle.py: SgdRig.step holds every launch to it), one captured launch
following two rates, the table walker, and the three captured steps with device_hyper=True against today's by-value steps bit
for bit, without a re-capture on set_lr / new_epoch.  Reference: MultiStepLR (cdf_alignment_admm/resnet-20-cifar-10/main.py:97,126),
the per-epoch SGD and the per-iteration alpha / lambd of the Office trees (dann_office/main.py:321-328,345-348; dsan_office/
main.py:316-329,381-382,410)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_weights_cpu as C
from tests.conftest import load_golden
from tests.test_gpu_dsan import differing, full_state
from tests.test_gpu_weights_optim import SENTINEL, Arena, SgdRig, bits_equal, done, three_steps

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from det_init import det_init_, sample  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the launchers
class Hyper:
    """lr and fresh as two guarded one-element windows of device memory (the kernels only read them)"""

    def __init__(self, dev):
        self.arena = Arena(dev, [1, 1])
        self.lr, self.fresh = self.arena.views
        self.set(0.0, 0.0)

    def set(self, lr=None, fresh=None):
        if lr is not None:
            self.lr.fill_(float(lr))            # double -> float32, round to nearest: what a by-value `float` argument gets
        if fresh is not None:
            self.fresh.fill_(float(fresh))

    def check(self):
        self.arena.get()                        # guards intact


def dev_prefix(rig, hyper, firsts, bitW, h, with_fresh=True):
    L = rig.L
    pre = rig.prefix(hyper, firsts, bitW)       # (T, p, g, buf, n, cdf, pdf, first, lr, mom, damp, wd, nest, bitW, lam, lam2)
    h.set(lr=pre[8])
    return pre[:8] + (L.ptr(h.lr), L.ptr(h.fresh) if with_fresh else None) + pre[9:]


def sgd_dev_launch(rig, h, with_fresh=True):
    def launch(hyper, firsts, bitW):
        done(rig.lib.alignq_sgd_step_multi_dev(*dev_prefix(rig, hyper, firsts, bitW, h, with_fresh), rig.L.stream_ptr()),
             "alignq_sgd_step_multi_dev")
    return launch


def site_arena(dev, S):
    site = Arena(dev, [64] * (3 * S))
    rng = np.random.default_rng(S)
    site.put([(0.1 * rng.standard_normal(64)).astype(np.float32) for _ in range(3 * S)])
    return site


def admm_launch(rig, site, S, h=None, with_fresh=True):
    """alignq_sgd_admm_step_multi (h None) or its _dev form with S sites of dim = b = 8"""
    D, A, G = site.views[:S], site.views[S:2 * S], site.views[2 * S:]

    def launch(hyper, firsts, bitW):
        L = rig.L
        tail = (S, L.ptr_array(D), L.ptr_array(A), L.ptr_array(G), 8, 8, 0.2, 0.3, L.stream_ptr())
        if h is None:
            done(rig.lib.alignq_sgd_admm_step_multi(*rig.prefix(hyper, firsts, bitW), *tail), "alignq_sgd_admm_step_multi")
        else:
            done(rig.lib.alignq_sgd_admm_step_multi_dev(*dev_prefix(rig, hyper, firsts, bitW, h, with_fresh), *tail),
                 "alignq_sgd_admm_step_multi_dev")
    return launch


def assert_runs_equal(ra, rb):
    for s0, s1 in zip(ra, rb):
        for a0, a1 in zip(s0, s1):              # p, g, buf
            assert all(bits_equal(x, y) for x, y in zip(a0, a1))


def fresh_step(rig, launch_firsts0, hyper, bitW):
    """one launch with every first = 0 on NaN-poisoned buffers (the caller's launch has fresh = 1 staged): (p, g, buf)"""
    rig.g.put([gs[0] for _, gs, _, _ in rig.inputs])
    rig.buf.put([np.full(n, np.nan, np.float32) for n in rig.sizes])
    launch_firsts0(hyper, [0] * rig.T, bitW)
    return rig.p.get(), rig.g.get(), rig.buf.get()


@pytest.mark.parametrize("hi", range(len(C.SGD_HYPER)))
@pytest.mark.parametrize("lname", ["six", "t73"])
def test_sgd_dev_launcher_equals_the_by_value_launcher_bit_for_bit(dev, lname, hi):
    """three_steps (first = 1 everywhere on poisoned buffers, a live step, `first` mixed) through alignq_sgd_step_multi_dev with
    fresh = 0 (a NULL fresh_dev for every second hyper set): SgdRig.step's float64 bars hold, and p / g / buf equal the by-value
    launcher's bit for bit; then fresh = 1 with every first = 0 on poisoned buffers equals the by-value first step."""
    hyper, bitW = C.SGD_HYPER[hi], (2, 4, 8)[hi % 3]
    sizes, seed = C.SGD_LISTS[lname], C._seed(lname)
    ref = SgdRig(dev, sizes, seed)
    want = three_steps(ref, ref.launch_multi, hyper, bitW)
    rig, h = SgdRig(dev, sizes, seed), Hyper(dev)
    got = three_steps(rig, sgd_dev_launch(rig, h, with_fresh=hi % 2 == 0), hyper, bitW)
    assert_runs_equal(want, got)
    rig2 = SgdRig(dev, sizes, seed)
    h.set(fresh=1.0)
    p, g, buf = fresh_step(rig2, sgd_dev_launch(rig2, h), hyper, bitW)
    for got_t, want_t in zip((p, g), want[0][:2]):
        assert all(bits_equal(x, y) for x, y in zip(got_t, want_t))
    if hyper[1] != 0:
        assert all(bits_equal(x, y) for x, y in zip(buf, want[0][2]))
        assert not any(np.isnan(b).any() for b in buf)
    h.check()


@pytest.mark.parametrize("hi", range(len(C.SGD_HYPER)))
@pytest.mark.parametrize("lname,S", [("six", 2), ("t73", 1)])
def test_sgd_admm_dev_launcher_equals_the_by_value_launchers_bit_for_bit(dev, lname, S, hi):
    """alignq_sgd_admm_step_multi_dev: the SGD role equals alignq_sgd_step_multi, both roles equal alignq_sgd_admm_step_multi, bit
    for bit; 73 parameters take the fall-back to the two separate calls in both forms."""
    hyper, bitW = C.SGD_HYPER[hi], (8, 4, 2)[hi % 3]
    sizes, seed = C.SGD_LISTS[lname], C._seed(lname)
    plain = SgdRig(dev, sizes, seed)
    want = three_steps(plain, plain.launch_multi, hyper, bitW)
    ref, ref_site = SgdRig(dev, sizes, seed), site_arena(dev, S)
    want_admm = three_steps(ref, admm_launch(ref, ref_site, S), hyper, bitW)
    rig, site, h = SgdRig(dev, sizes, seed), site_arena(dev, S), Hyper(dev)
    got = three_steps(rig, admm_launch(rig, site, S, h, with_fresh=hi % 2 == 1), hyper, bitW)
    assert_runs_equal(want, got)
    assert_runs_equal(want_admm, got)
    sites_want, sites_got = ref_site.get(), site.get()
    assert all(bits_equal(a, b) for a, b in zip(sites_want, sites_got))
    assert not all(bits_equal(a, b) for a, b in zip(sites_got[S:], site_arena(dev, S).get()[S:]))      # (the site role ran)
    rig2, site2 = SgdRig(dev, sizes, seed), site_arena(dev, S)
    h.set(fresh=1.0)
    p, g, buf = fresh_step(rig2, admm_launch(rig2, site2, S, h), hyper, bitW)
    for got_t, want_t in zip((p, g) + ((buf,) if hyper[1] != 0 else ()), want[0]):
        assert all(bits_equal(x, y) for x, y in zip(got_t, want_t))
    h.check()


# ------------------------------------------------------------------------------------------------ 2. one graph, two rates
def test_one_captured_launch_follows_the_rate_in_device_memory(dev):
    """one alignq_sgd_step_multi_dev launch (T = 6) in a graph, replayed with lr = a and, written between the replays, lr = b:
    the two by-value launches' p, g and buf bit for bit"""
    lr_a, lr_b = 0.04, 0.004
    _, mom, damp, wd, nest = C.SGD_HYPER[0]
    sizes, seed, bitW = C.SGD_LISTS["six"], C._seed("six"), 8
    rigs = [SgdRig(dev, sizes, seed) for _ in range(2)]
    for rig in rigs:
        rig.g.put([gs[0] for _, gs, _, _ in rig.inputs])
        rig.buf.put([gs[2] for _, gs, _, _ in rig.inputs])             # live momentum buffers (first = 0 is baked into the graph)
    ref, rig = rigs
    for lr in (lr_a, lr_b):
        ref.launch_multi((lr, mom, damp, wd, nest), [0] * ref.T, bitW)
    h = Hyper(dev)
    args = dev_prefix(rig, (lr_a, mom, damp, wd, nest), [0] * rig.T, bitW, h)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.L.check(rig.lib.alignq_sgd_step_multi_dev(*args, rig.L.stream_ptr()), "alignq_sgd_step_multi_dev")
    h.set(lr=lr_a)
    graph.replay()
    h.set(lr=lr_b)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in ((ref.p, rig.p), (ref.g, rig.g), (ref.buf, rig.buf)):
        assert all(bits_equal(x, y) for x, y in zip(a.get(), b.get()))
    assert not bits_equal(ref.p.get()[3], ref.p_host[3])                  # (the steps moved the parameters)
    h.check()


# ------------------------------------------------------------------------------------------------ 3. the table walker
def test_hyper_advance_walks_the_table_and_clamps(dev):
    from alignq_amd import _lib as L
    lib = L.load()
    rows, cols = 5, 7
    table_host = (np.arange(rows * cols, dtype=np.float32) * 1.25 + 0.5)
    tab, out = Arena(dev, [rows * cols]), Arena(dev, [cols])
    tab.put([table_host])
    cur = torch.tensor([SENTINEL, 0, SENTINEL], dtype=torch.int32, device=dev)

    def launch():
        return lib.alignq_hyper_advance(L.ptr(tab.views[0]), rows, cols, cur.data_ptr() + 4, L.ptr(out.views[0]), L.stream_ptr())

    def check(i):
        want = table_host.reshape(rows, cols)[min(i, rows - 1)]
        assert bits_equal(out.get()[0], want), (i, out.get()[0], want)
        assert cur.tolist() == [SENTINEL, i + 1, SENTINEL]

    for i in range(7):
        done(launch(), "alignq_hyper_advance")
        check(i)
    assert bits_equal(tab.get()[0], table_host)
    # the same as a node of a graph
    out.reset()
    cur[1] = 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(launch(), "alignq_hyper_advance")
    assert cur.tolist()[1] == 0                                            # (capturing runs nothing)
    for i in range(7):
        graph.replay()
        torch.cuda.synchronize()
        check(i)
    assert bits_equal(tab.get()[0], table_host)


# ------------------------------------------------------------------------------------------------ 4. ResNet-20
@pytest.mark.parametrize("tree", ["admm", "cdf"])
def test_resnet20_device_hyper_keeps_its_graph_across_set_lr(dev, tree):
    """ResNet-20 8W/8A, B = 128: capture(warmup=2), two replays, set_lr(lr / 10), two replays - by value (re-captured), with the
    rate in device memory (the same graph object) and driven by a multistep table without any set_lr: one state, bit for bit."""
    from alignq_amd import config
    from alignq_amd.resnet import resnet20_quant
    from alignq_amd.schedule import multistep
    from alignq_amd.train_step import TrainStep
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size)
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    try:
        gen = torch.Generator().manual_seed(13)
        x = torch.randn(128, 3, 32, 32, generator=gen).to(dev)
        y = torch.randint(0, 10, (128,), generator=gen).to(dev)
        lr = 0.04
        table = multistep(lr, [2], 0.1, 3, 2)             # 2 iterations per "epoch": rows 0-3 at lr, rows 4-5 at lr * 0.1
        assert table.shape == (6, 4)
        assert np.float32(lr / 10) == table[4, 0].item() == table[5, 0].item() and table[3, 0].item() == np.float32(lr)
        states, steps = [], []
        for mode in ("value", "device", "table"):
            torch.manual_seed(7)
            m = det_init_(resnet20_quant(8, 8, tree=tree)).to(dev).train()
            s = TrainStep(m, lr=lr, channels_last=True, qconv=True, fuse_bn=True, device_hyper=mode != "value")
            assert bool(s.admms) == (tree == "admm")
            if mode == "table":
                s.set_schedule(table)
            s.capture(x, y, warmup=2)
            graph = s._graph
            assert graph is not None and s._graph2 is None
            for _ in range(2):
                s(x, y)
            if mode != "table":
                s.set_lr(lr / 10)
            assert (s._graph is graph) == (mode != "value")
            assert all(g["lr"] == lr / 10 for g in s.optimizer_t.param_groups) or mode == "table"
            for _ in range(2):
                out = s(x, y)
            torch.cuda.synchronize()
            assert torch.isfinite(out[1])
            if mode != "value":
                assert s._graph is graph
                hyper = s.current_hyper()
                assert hyper["lr"] == [float(np.float32(lr / 10))] and hyper["fresh"] == 0.0
                assert hyper["cursor"] == (6 if mode == "table" else None)
            states.append(full_state(m, s, s.admms))
            steps.append(s)
        with pytest.raises(RuntimeError):
            steps[2].set_lr(lr)                          # the table owns the row
        for other, name in zip(states[1:], ("device", "table")):
            bad = differing(states[0], other)
            assert not bad, "%s mode differs from the by-value step in %d tensors, first: %s" % (name, len(bad), bad[:6])
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size = old


# ------------------------------------------------------------------------------------------------ 5. tiny DANN / DSAN
def tiny_net(kind, stage):
    from alignq_amd.resnet_office import DANN, DSAN, Bottleneck, ResNet
    cls = DANN if kind == "dann" else DSAN
    return cls(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, stage)


def reference_bars(kind, g, it, step, named, outs, init_state, prev):
    """The bars of test_office_tiny_dann_two_iterations_vs_reference (tests/test_gpu_round2.py, fixture G10) and of
    test_office_tiny_dsan_two_iterations_vs_reference (tests/test_gpu_dsan.py, fixture G16) for iteration `it`."""
    if kind == "dann":
        cls_s, loss, tl = outs
        if it == 0:
            np.testing.assert_allclose(npy(cls_s), g["cls_s_0"], atol=0.2)
        np.testing.assert_allclose(float(tl), float(g[f"tl_s_{it}"]) + float(g[f"tl_t_{it}"]), rtol=2e-4)
        np.testing.assert_allclose(float(loss), float(g[f"loss_{it}"]), rtol=2e-2)
        heads = ("class_classifier", "domain_classifier")
    else:
        s_pred, loss, loss_mmd = outs
        if it == 0:
            np.testing.assert_allclose(npy(s_pred), g["s_pred_0"], atol=0.2)
        np.testing.assert_allclose(npy(loss_mmd), g[f"loss_mmd_{it}"], rtol=2e-2)
        np.testing.assert_allclose(npy(loss), g[f"loss_{it}"], rtol=2e-2)
        heads = ("bottle", "cls_fc")
    for bi, b in enumerate(step.blocks):
        D = npy(b.admm0.D)
        d_tgt = np.abs(D - g[f"D_{it}_{bi}"]).max()
        assert d_tgt < (6e-3, 3e-2)[it], (it, bi, d_tgt)                                  # the TARGET pass's D
        if kind == "dann":
            assert d_tgt < 0.4 * np.abs(D - g[f"Dsrc_{it}_{bi}"]).max(), (it, bi)
    for j, (n, p) in enumerate(named):
        tol = (6e-3, 2e-2)[it] if ("alterD" in n or "gamma" in n) else (2.5e-3, 8e-3)[it]
        np.testing.assert_allclose(npy(sample(p)), g[f"after_{it}/{j}"], atol=tol, err_msg=n)
    for j, (n, p) in enumerate(named):
        if not n.startswith(heads) or p.dim() != 2:
            continue
        prev_ref = g[f"after_{it - 1}/{j}"] if it else npy(sample(init_state[n]))
        prev_got = prev[n] if it else npy(sample(init_state[n]))
        d_ref, d_got = g[f"after_{it}/{j}"] - prev_ref, npy(sample(p)) - prev_got
        cos = float((d_ref * d_got).sum() / (np.linalg.norm(d_ref) * np.linalg.norm(d_got) + 1e-30))
        ratio = float(np.linalg.norm(d_got) / (np.linalg.norm(d_ref) + 1e-30))
        assert cos > (0.99, 0.8)[it] and abs(ratio - 1.0) < (0.05, 0.3)[it], (n, it, cos, ratio)
        buf = npy(sample(step.optimizer_t.state[p]["momentum_buffer"]))
        rb = float(np.linalg.norm(buf) / (np.linalg.norm(g[f"buf_{it}/{j}"]) + 1e-30))
        assert abs(rb - 1.0) < (0.05, 0.3)[it], (n, it, rb)
    return {n: npy(sample(p)) for n, p in named}


def never_stepped(model, step, state):
    """Momentum buffers of parameters no backward reaches (the ResNet's unused fc): SGD.attach_hyper creates every buffer up
    front, the by-value optimizer only those of parameters that have a gradient.  They must still be the zeros they were made as."""
    out = []
    for n, p in model.named_parameters():
        key = "momentum:" + n
        if p.grad is None and key in state:
            assert not state[key].any(), n
            out.append(key)
    return out


@pytest.mark.parametrize("kind", ["dann", "dsan"])
def test_office_tiny_device_hyper_follows_alpha_and_new_epoch_in_one_graph(dev, kind):
    """Twin A: today's eager step - alpha (lambd) by value in every call, new_epoch builds a new SGD.  Twin B: device_hyper=True,
    capture(warmup=2) once; alpha / lambd and new_epoch go through the device row, every iteration is a replay of ONE graph.
    Two epochs of two iterations with a different alpha / lambd in each: every parameter, buffer, momentum buffer and ADMM.D bit
    for bit (the stem's tensors, behind torch's atomic max-pool backward, to rounding).  Then twin B, put back to the initial
    state in place, replays the two iterations of fixture G10 / G16 and meets the reference bars of the existing tests.

    The tiny network's channel counts (8 .. 64) send its convolutions to MIOpen, whose default filter-gradient algorithms for
    these shapes use atomics: two runs of the SAME eager by-value step from one state differ in 55 of 183 tensors after one
    iteration (momentum of layer1.0.conv1.weight by 6.6e-7 of 0.69, measured on the MI355X), and at 4 bits such a difference can
    flip a bin.  A bit-for-bit comparison of two code paths therefore runs with torch's deterministic algorithms switched on, under
    which that control is bit-identical in all 183 tensors after each of six iterations.  The control is part of the test: a
    second by-value eager twin runs twin A's sequence and must equal it in every tensor, the stem's included."""
    from alignq_amd import config
    from alignq_amd.train_step import DSANTrainStep, OfficeTrainStep, dann_alpha, dsan_lambd
    g = load_golden("g10_office_tiny_dann" if kind == "dann" else "g16_office_tiny_dsan")
    g10 = g if kind == "dann" else load_golden(str(g["inputs"]))
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = 6
    old_param = config.args.param
    old_det = (torch.backends.cudnn.deterministic, torch.are_deterministic_algorithms_enabled(),
               torch.is_deterministic_algorithms_warn_only_enabled())
    try:
        torch.backends.cudnn.deterministic = True
        torch.use_deterministic_algorithms(True, warn_only=True)
        if kind == "dsan":
            config.args.param = float(g["param"])
        lr, num_epochs, iters = float(g["lr"]), int(g["num_epochs"]), 2
        batches = [(cu(g10["xs"][i], dev), cu(g["ys"][i], dev), cu(g10["xt"][i], dev)) for i in range(2)]
        if kind == "dann":
            warm = float(g["alpha"])
            ramp = {(e, i): dann_alpha(iters * e + i + 1, num_epochs, iters) for e in (1, 2) for i in range(iters)}
        else:
            warm = float(g["lambd"][0])
            ramp = {(e, i): dsan_lambd(iters * e + i, num_epochs, iters) for e in (1, 2) for i in range(iters)}
        assert len(set(ramp.values()) | {warm}) == 5

        def make(device_hyper):
            torch.manual_seed(0)
            net = tiny_net(kind, str(g["stage"]))
            assert [n for n, _ in net.named_parameters()] == list(g["names"])
            net = det_init_(net).to(dev).train()
            kw = dict(lr=lr, channels_last=True, fuse_relu=True, dual=True, device_hyper=device_hyper)
            step = OfficeTrainStep(net, alpha=warm, **kw) if kind == "dann" else DSANTrainStep(net, **kw)
            assert step.dual
            return net, step

        def call(step, batch, value, by_value):
            if kind == "dsan":
                return step(*batch, value)
            if by_value:
                step.alpha = value
                return step(*batch)
            return step(*batch, alpha=value)

        net_a, a = make(False)
        net_b, b = make(True)
        net_c, c = make(False)                              # the control: twin A's sequence once more
        keep = [(t, t.detach().clone()) for t in list(net_b.parameters()) + list(net_b.buffers())]
        init_state = {n: p.detach().clone() for n, p in net_b.named_parameters()}
        for _ in range(2):                                  # the two iterations twin B's capture warms up with
            call(a, batches[0], warm, True)
            call(c, batches[0], warm, True)
        if kind == "dann":
            b.capture(*batches[0], warmup=2)
        else:
            b.capture(*batches[0], warmup=2, lambd=warm)
        graph, opt_b = b._graph, b.optimizer_t
        assert graph is not None and b._graph2 is None
        for epoch in (1, 2):
            opt_a = a.optimizer_t
            ra = a.new_epoch(epoch, num_epochs, lr)
            rb = b.new_epoch(epoch, num_epochs, lr)
            c.new_epoch(epoch, num_epochs, lr)
            assert ra == rb and a.optimizer_t is not opt_a and b.optimizer_t is opt_b and b._graph is graph
            assert [gr["lr"] for gr in a.optimizer_t.param_groups] == [gr["lr"] for gr in b.optimizer_t.param_groups]
            for i in range(iters):
                call(a, batches[i], ramp[epoch, i], True)
                call(b, batches[i], ramp[epoch, i], False)
                call(c, batches[i], ramp[epoch, i], True)
                assert b._graph is graph
        torch.cuda.synchronize()
        hyper = b.current_hyper()
        rates = [gr["lr"] for gr in b.optimizer_t.param_groups]
        assert rates[0] == rb / 10 and all(r == rb for r in rates[1:]) and len(rates) == 3
        assert hyper["fresh"] == 0.0 and hyper["lr"] == [float(np.float32(v)) for v in rates]
        assert hyper["alpha" if kind == "dann" else "coef"] == float(np.float32(
            ramp[2, 1] if kind == "dann" else config.args.param * ramp[2, 1]))
        st_a, st_b = full_state(net_a, a, a.admms), full_state(net_b, b, b.admms)
        bad = differing(st_a, full_state(net_c, c, c.admms))
        assert not bad, "two runs of the by-value eager step differ in %d tensors, first: %s" % (len(bad), bad[:6])
        for key in never_stepped(net_b, b, st_b):
            assert key not in st_a
            st_b.pop(key)
        root = "feature." if kind == "dann" else "feature_layers."
        stem = (root + "conv1.", root + "bn1.")
        stem_keys = [k for k in st_a if k.split(":", 1)[1].startswith(stem)]
        assert stem_keys
        for key in stem_keys:
            np.testing.assert_allclose(st_a[key], st_b[key], rtol=1e-5, atol=1e-7 * float(np.abs(st_a[key]).max()) + 1e-12, err_msg=key)
            st_a.pop(key), st_b.pop(key)
        bad = differing(st_a, st_b)
        assert not bad, "the device-hyper graph differs from the by-value eager step in %d tensors, first: %s" % (len(bad), bad[:6])
        if kind == "dann":
            with pytest.raises(RuntimeError, match="device_hyper"):
                a.capture(*batches[0], warmup=0)(*batches[0], alpha=0.25)
        # ---- twin B against the reference's own numbers: the initial state put back IN PLACE (the graph's addresses), then the
        # fixture's two iterations (epochs 1 and 2, one iteration each) as replays
        with torch.no_grad():
            for t, c in keep:
                t.copy_(c)
        named = list(net_b.named_parameters())
        prev = None
        for it, epoch in enumerate((1, 2)):
            rate = b.new_epoch(epoch, num_epochs, lr)
            assert abs(rate - float(g[f"rate_{it}"])) < 1e-12
            outs = call(b, batches[it], float(g["alpha"]) if kind == "dann" else float(g["lambd"][it]), False)
            torch.cuda.synchronize()
            assert b._graph is graph and b.optimizer_t is opt_b
            prev = reference_bars(kind, g, it, b, named, outs, init_state, prev)
    finally:
        torch.backends.cudnn.deterministic = old_det[0]
        torch.use_deterministic_algorithms(old_det[1], warn_only=old_det[2])
        config.args.param = old_param
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100
