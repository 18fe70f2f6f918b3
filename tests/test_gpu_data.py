"""GPU checks of the device input pipeline (include/alignq.h: alignq_data_batch; alignq_amd/data.py).

The kernel against tests/data_oracle.py (the NumPy statement of the header's specification) BIT FOR BIT: the kernel does no
floating-point arithmetic (a table gather), so there is no tolerance to choose.  The loader inside a captured step against a
second, identically initialised step that is fed the oracle's batches through static_inputs(): the repository's
replay == eager tests (test_gpu_round6.py) establish that this comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import data_oracle as DO

pytestmark = pytest.mark.gpu

SENTINEL_X, SENTINEL_Y = 0x7FC12345, -7          # a NaN payload no table holds; no label is negative


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synthetic(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, n).astype(np.int64)


def launch(dev, ds, perm_t, epoch, first, B, rank, world, seed, nhwc, advance=0):
    """One alignq_data_batch launch into sentinel-filled tensors; returns (x as NCHW-indexed numpy, y numpy)"""
    from alignq_amd import _lib as L
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = torch.empty(B, 3, 32, 32, dtype=torch.float32, device=dev).contiguous(memory_format=fmt)
    x.view(torch.int32).fill_(SENTINEL_X)
    y = torch.full((B,), SENTINEL_Y, dtype=torch.int64, device=dev)
    cursor = torch.tensor([epoch, first, 0, 0], dtype=torch.int32).to(dev)
    rc = L.load().alignq_data_batch(L.ptr(ds.images), L.ptr(ds.labels), L.ptr(perm_t), L.ptr(cursor), advance, L.ptr(ds.lut), len(ds), B,
                                    rank, world, seed, ds.pad, int(ds.flip), L.ptr(x), int(nhwc), L.ptr(y), L.stream_ptr())
    assert rc == 0, rc
    # advance = 0: the cursor is only read; else the launch moved it on and left its ticket at 0
    assert cursor.cpu().tolist() == [epoch, first + advance, 0, 0]
    return x.cpu().numpy(), y.cpu().numpy()


@pytest.mark.parametrize("nhwc", [0, 1], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("augment", [True, False], ids=["augment", "plain"])
def test_kernel_equals_numpy_oracle_bit_for_bit(dev, nhwc, augment):
    from alignq_amd import data as D
    n = 1000
    images, labels = synthetic(n, 17)
    ds = D.DeviceImages.preset("cifar10_train" if augment else "cifar10_test", images, labels, dev)
    lut = DO.normalise_table(D.CIFAR10_MEAN, D.CIFAR10_STD)
    assert np.array_equal(bits(ds.lut.cpu().numpy()), bits(lut))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    perm_t = perm.to(dev)
    seed, epoch = 0xDEADBEEF12345678, 6
    n_checked = 0
    #       first  B   rank world
    cases = [(0, 128, 0, 1), (384, 80, 0, 1), (999, 1, 0, 1), (517, 1, 0, 1),
             (256, 128, 0, 2), (256, 128, 1, 2),
             (950, 128, 0, 1), (950, 80, 0, 1), (960, 20, 1, 2), (900, 128, 1, 2)]      # the last batch of the epoch: rows past N
    for with_perm in (True, False):
        for first, B, rank, world in cases:
            x, y = launch(dev, ds, perm_t if with_perm else None, epoch, first, B, rank, world, seed, nhwc,
                          advance=world * B if with_perm else 0)
            ex, ey = DO.batch(images, labels, perm.numpy() if with_perm else None, lut, first, B, rank, world, seed, epoch,
                              ds.pad, ds.flip)
            rows = ex.shape[0]
            assert rows == max(0, min(B, n - (first + rank * B)))
            bad = int((bits(x[:rows]) != bits(ex)).sum())
            assert bad == 0, "%d of %d elements differ (first %d B %d rank %d/%d perm %s)" % (bad, ex.size, first, B, rank, world, with_perm)
            assert np.array_equal(y[:rows], ey)
            # rows past the end of the epoch are untouched
            assert (bits(x[rows:]) == SENTINEL_X).all() and (y[rows:] == SENTINEL_Y).all()
            n_checked += 1
    assert n_checked == 20
    if augment:      # the draws did something: a plain batch differs
        plain = D.DeviceImages.preset("cifar10_test", images, labels, dev)
        x0, _ = launch(dev, plain, perm_t, epoch, 0, 128, 0, 1, seed, nhwc)
        x1, _ = launch(dev, ds, perm_t, epoch, 0, 128, 0, 1, seed, nhwc)
        assert (bits(x0) != bits(x1)).any()


def test_loader_epoch_iteration_and_captured_fill(dev):
    """DeviceLoader: one epoch by iteration (391-style: full batches and the short one) equals the oracle; a HIP graph that holds
    ONLY the fill produces batch n on its n-th replay after begin_epoch, across epochs, with the same graph."""
    from alignq_amd import data as D
    n, B = 3 * 64 + 40, 64
    images, labels = synthetic(n, 23)
    lut = DO.normalise_table(D.CIFAR10_MEAN, D.CIFAR10_STD)
    ds = D.DeviceImages.preset("cifar10_train", images, labels, dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.DeviceLoader(ds, B).fill(torch.empty(B, 3, 32, 32), torch.empty(B, dtype=torch.int64))
    for channels_last in (False, True):
        loader = D.DeviceLoader(ds, B, seed=9, channels_last=channels_last)
        assert len(loader) == 4 and loader.shuffle
        perms = {}
        for epoch in (0, 1):
            if epoch:
                loader.begin_epoch(epoch)
            perms[epoch] = loader.perm.cpu().numpy().copy()
            assert np.array_equal(np.sort(perms[epoch]), np.arange(n))
            got = [(x.clone(), y.clone()) for x, y in loader]
            assert [g[0].shape[0] for g in got] == [64, 64, 64, 40]
            assert all(g[0].is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format) for g in got)
            for k, (x, y) in enumerate(got):
                ex, ey = DO.batch(images, labels, perms[epoch], lut, k * B, x.shape[0], 0, 1, 9, epoch, 4, True)
                assert np.array_equal(bits(x.cpu().numpy()), bits(ex)) and np.array_equal(y.cpu().numpy(), ey), (epoch, k)
            assert loader.cursor.cpu().tolist() == [epoch, n, 0, 0] and loader.next_batch() is None
        assert not np.array_equal(perms[0], perms[1])
        # the same (seed, epoch) repeats the order; iterating again starts the next epoch by itself
        loader.begin_epoch(0)
        assert np.array_equal(loader.perm.cpu().numpy(), perms[0])

        # a graph holding only the fill
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        sx = torch.zeros(B, 3, 32, 32, device=dev).contiguous(memory_format=fmt)
        sy = torch.zeros(B, dtype=torch.int64, device=dev)
        perm_ptr, cursor_ptr = loader.perm.data_ptr(), loader.cursor.data_ptr()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loader.record(sx, sy)
        for epoch in (0, 1, 0):
            loader.begin_epoch(epoch)
            assert (loader.perm.data_ptr(), loader.cursor.data_ptr()) == (perm_ptr, cursor_ptr)      # rewritten in place
            for k in range(3):
                graph.replay()
                ex, ey = DO.batch(images, labels, perms[epoch], lut, k * B, B, 0, 1, 9, epoch, 4, True)
                assert np.array_equal(bits(sx.cpu().numpy()), bits(ex)) and np.array_equal(sy.cpu().numpy(), ey), (epoch, k)
                assert loader.cursor.cpu().tolist() == [epoch, (k + 1) * B, 0, 0]


def full_state(model, step):
    st = {}
    for n_, p in model.named_parameters():
        st["param:" + n_] = p.detach().clone()
    for n_, b in model.named_buffers():
        st["buffer:" + n_] = b.detach().clone()
    names = {id(p): n_ for n_, p in model.named_parameters()}
    for p, s in step.optimizer_t.state.items():
        if s.get("momentum_buffer") is not None:
            st["momentum:" + names[id(p)]] = s["momentum_buffer"].detach().clone()
    for i, a in enumerate(step.admms):
        if a.D is not None:
            st["D:%d" % i] = a.D.detach().clone()
    return st


def same_tensor_bits(a, b):
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def assert_same_outputs(o1, o2, where):
    for k, (a, b) in enumerate(zip(o1, o2)):
        if torch.is_tensor(a):
            assert same_tensor_bits(a, b), "output %d differs at %s" % (k, where)


CASES = [("tiny_4bit_admm", None, 4, "admm"), ("resnet20_8bit_admm", 20, 8, "admm"), ("resnet20_8bit_cdf", 20, 8, "cdf")]


@pytest.mark.parametrize("name,depth,nbits,tree", CASES, ids=[c[0] for c in CASES])
def test_train_step_with_loader_in_graph_equals_step_fed_oracle_batches(dev, name, depth, nbits, tree):
    """Two epochs of a 336-image set at batch 128 (two replays and the short batch of 80 through the eager fallback per epoch; the
    second epoch returns to the graph): logits, both losses at every step and every parameter, buffer, momentum and ADMM.D at the
    end equal, bit for bit, those of a twin step that replays its graph on the oracle's batches written into static_inputs()."""
    from alignq_amd import config, data as D
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet, resnet20_quant
    from alignq_amd.train_step import TrainStep
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size)
    config.args.bitW = config.args.abitW = nbits
    config.args.train_batch_size = 128
    try:
        n, B, seed = 2 * 128 + 80, 128, 4
        images, labels = synthetic(n, 31)
        lut = DO.normalise_table(D.CIFAR10_MEAN, D.CIFAR10_STD)
        ds = D.DeviceImages.preset("cifar10_train", images, labels, dev)
        loader = D.DeviceLoader(ds, B, seed=seed)

        def make():
            torch.manual_seed(7)
            if depth is None:
                net = PreActResNet(PreActBlock_conv_Q, [1, 1, 1], nbits, nbits, "second", 10, tree=tree)
            else:
                net = resnet20_quant(nbits, nbits, tree=tree)
            return net.to(dev).train()
        m1, m2 = make(), make()
        s1 = TrainStep(m1, channels_last=True, qconv=True).set_producer(loader)
        s2 = TrainStep(m2, channels_last=True, qconv=True)
        x0, y0 = loader.peek()
        ex0, ey0 = DO.batch(images, labels, loader.perm.cpu().numpy(), lut, 0, B, 0, 1, seed, 0, 4, True)
        assert np.array_equal(bits(x0.cpu().numpy()), bits(ex0)) and np.array_equal(y0.cpu().numpy(), ey0)
        assert loader.cursor.cpu().tolist() == [0, 0, 0, 0]              # peek consumes nothing
        s1.capture(x0, y0, warmup=3)
        s2.capture(x0, y0, warmup=3)
        assert s1._graph is not None and s1._graph2 is None and s2._graph2 is None
        with pytest.raises(RuntimeError, match="next"):
            s1(*s1.static_inputs())                                      # the graph fills its own inputs
        sx, sy = s2.static_inputs()
        for epoch in (0, 1):
            if epoch == 1:
                s1.set_lr(0.02), s2.set_lr(0.02)                         # re-capture keeps the producer
                assert s1._producer is loader and s1._graph is not None
                sx, sy = s2.static_inputs()
            loader.begin_epoch(epoch)
            perm = loader.perm.cpu().numpy().copy()
            for k in range(len(loader)):
                rows = loader.next_batch_size()
                assert rows == (128 if k < 2 else 80)
                o1 = s1.next()
                ex, ey = DO.batch(images, labels, perm, lut, k * B, rows, 0, 1, seed, epoch, 4, True)
                if rows == B:
                    sx.copy_(torch.from_numpy(ex).to(dev))
                    sy.copy_(torch.from_numpy(ey).to(dev))
                    o2 = s2(sx, sy)
                    got_x, got_y = s1.static_inputs()
                    assert np.array_equal(bits(got_x.cpu().numpy()), bits(ex)) and np.array_equal(got_y.cpu().numpy(), ey)
                else:
                    o2 = s2(torch.from_numpy(ex).to(dev), torch.from_numpy(ey).to(dev))
                assert torch.isfinite(o1[1])
                assert_same_outputs(o1, o2, "epoch %d batch %d" % (epoch, k))
            assert loader.next_batch_size() == 0
            with pytest.raises(RuntimeError, match="exhausted"):
                s1.next()
        # train_epoch drives the same loop
        o1 = D.train_epoch(s1, loader, 2)
        loader2 = D.DeviceLoader(ds, B, seed=seed)
        o2 = D.train_epoch(s2, loader2, 2)            # a step without a producer: the loader's batches through step(x, y)
        assert_same_outputs(o1, o2, "train_epoch")
        torch.cuda.synchronize()
        st1, st2 = full_state(m1, s1), full_state(m2, s2)
        assert st1.keys() == st2.keys()
        bad = [key for key in st1 if not same_tensor_bits(st1[key], st2[key])]
        assert not bad, "%d tensors differ, first: %s" % (len(bad), bad[:6])
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size = old


def graph_nodes(graph):
    """Number of nodes of a captured torch.cuda.CUDAGraph(keep_graph=True), from the HIP runtime"""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n))
    assert rc == 0, rc
    return int(n.value)


def test_graph_without_producer_is_unchanged_and_producer_adds_one_node(dev, monkeypatch):
    """The headline step (ResNet-20 8W/8A CDF+ADMM, batch 128, channels-last) captured WITHOUT a producer is the graph of 83 nodes
    DESIGN.md records for it, and step(x, y) replays it as before; with a loader attached the graph holds ONE node more (the batch
    launch, which also moves the cursor on)."""
    from alignq_amd import config, data as D
    from alignq_amd.resnet import resnet20_quant
    from alignq_amd.train_step import TrainStep
    plain = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: plain(keep_graph=True))
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size)
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    try:
        images, labels = synthetic(512, 3)
        ds = D.DeviceImages.preset("cifar10_train", images, labels, dev)
        loader = D.DeviceLoader(ds, 128, seed=1)
        counts = []
        for with_loader in (False, True):
            torch.manual_seed(7)
            step = TrainStep(resnet20_quant(8, 8).to(dev).train(), channels_last=True, qconv=True)
            if with_loader:
                step.set_producer(loader)
            x0, y0 = loader.peek()
            step.capture(x0, y0, warmup=3)
            counts.append(graph_nodes(step._graph))
            if with_loader:
                loader.begin_epoch(0)
                out = step.next()
            else:
                assert step._producer is None
                before = step.model.logit.weight.detach().clone()
                out = step(x0, y0)
                assert out is step._outs and not torch.equal(before, step.model.logit.weight)      # a replay, and it trained
            torch.cuda.synchronize()
            assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]) and torch.isfinite(out[2])
        print("graph nodes: %d without a producer, %d with the loader" % tuple(counts))
        assert counts[0] == 83
        assert counts[1] == counts[0] + 1
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size = old


def test_evaluate_equals_eval_step_fed_the_same_tensors(dev):
    """evaluate(EvalStep, test loader) - by iteration and with the loader inside the captured graph - gives the counts of an EvalStep
    that is fed the oracle's normalised tensors batch by batch (340 images at batch 100: three full batches and one of 40)."""
    from alignq_amd import config, data as D
    from alignq_amd.eval_step import EvalStep
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    from alignq_amd.train_step import TrainStep
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size)
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = 128
    try:
        n, B = 340, 100
        images, labels = synthetic(n, 41)
        lut = DO.normalise_table(D.CIFAR10_MEAN, D.CIFAR10_STD)
        test_set = D.DeviceImages.preset("cifar10_test", images, labels, dev)
        loader = D.DeviceLoader(test_set, B)
        assert not loader.shuffle and len(loader) == 4
        torch.manual_seed(3)
        net = PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 4, 4, "second", 10).to(dev).train()
        step = TrainStep(net, channels_last=True, qconv=True)
        train_set = D.DeviceImages.preset("cifar10_train", images, labels, dev)
        for x, y in D.DeviceLoader(train_set, 128, seed=2):              # running statistics away from their initial values
            step(x, y)
        batches = [DO.batch(images, labels, None, lut, k * B, min(B, n - k * B), 0, 1, 0, 0, 0, False) for k in range(4)]
        ev = EvalStep(net, channels_last=True, qconv=True)
        with ev:
            for ex, ey in batches:
                ev(torch.from_numpy(ex).to(dev), torch.from_numpy(ey).to(dev))
            expected, expected_counts = ev.result(), ev.counts()
        assert expected_counts[3] == n
        got = D.evaluate(ev, loader)
        assert got == expected, (got, expected)
        assert net.training and ev._saved is None
        # the loader inside the evaluation graph
        ev.set_producer(loader)
        with ev:
            ev.capture(*loader.peek(), warmup=2)
            got_captured = D.evaluate(ev, loader)
            assert ev._graph is not None and ev.counts() == expected_counts
            again = D.evaluate(ev, loader)                               # accumulates: begin() zeroes, evaluate does not
            assert again[3] == 2 * n
        assert got_captured == expected, (got_captured, expected)
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size = old
