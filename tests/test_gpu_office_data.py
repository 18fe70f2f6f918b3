"""GPU checks of the Office input pipeline (include/alignq.h: alignq_data_crop_batch; alignq_amd/data.py: DeviceImages with a crop,
PairLoader; OfficeTrainStep / DSANTrainStep.set_producer).

The kernel against tests/office_data_oracle.py (the NumPy statement of the header's specification) BIT FOR BIT: the kernel does
no floating-point arithmetic (a table gather), so there is no tolerance to choose.  The pair loader inside a captured Office step
against a twin step that is called with the oracle's batches, by the rule of tests/test_gpu_schedule.py (deterministic
algorithms on, the stem's tensors behind torch's atomic max-pool backward to rounding, everything else bit for bit, and a control
twin that repeats the first twin's sequence and must equal it)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import office_data_oracle as OO
from tests.test_gpu_dsan import differing, full_state
from tests.test_gpu_schedule import tiny_net

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from det_init import det_init_  # noqa: E402

SENTINEL_X, SENTINEL_Y = 0x7FC12345, -7          # a NaN payload no table holds; no label is negative
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lut():
    return OO.normalise_table(MEAN, STD)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synthetic(n, side, seed, classes=31):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, side, side, 3), dtype=np.uint8), rng.integers(0, classes, n).astype(np.int64)


def device_set(images, labels, crop, train, dev):
    """The office_train / office_test pipeline at another crop size (the presets fix 224)"""
    from alignq_amd import data as D
    return D.DeviceImages(images, labels, MEAN, STD, device=dev, flip=train, shuffle=train, crop=crop,
                          window="random" if train else "center")


def launch(dev, ds, perm_t, epoch, first, B, rank, world, seed, nhwc, advance):
    """One alignq_data_crop_batch launch into sentinel-filled tensors; returns (x as NCHW-indexed numpy, y numpy)"""
    from alignq_amd import _lib as L
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = torch.empty(B, 3, ds.crop, ds.crop, dtype=torch.float32, device=dev).contiguous(memory_format=fmt)
    x.view(torch.int32).fill_(SENTINEL_X)
    y = torch.full((B,), SENTINEL_Y, dtype=torch.int64, device=dev)
    cursor = torch.tensor([epoch, first, 0, 0], dtype=torch.int32).to(dev)
    rc = L.load().alignq_data_crop_batch(L.ptr(ds.images), L.ptr(ds.labels), L.ptr(perm_t), L.ptr(cursor), advance, L.ptr(ds.lut), len(ds),
                                         ds.side, ds.crop, ds.span, ds.off0, B, rank, world, seed, int(ds.flip), L.ptr(x), int(nhwc),
                                         L.ptr(y), L.stream_ptr())
    assert rc == 0, rc
    # advance = 0: the cursor is only read; else the launch moved it on and left its ticket at 0 (re-armed)
    assert cursor.cpu().tolist() == [epoch, first + advance, 0, 0]
    return x.cpu().numpy(), y.cpu().numpy()


def check_rows(x, y, ex, ey, kept, where):
    rows = ex.shape[0]
    bad = int((bits(x[:rows][kept]) != bits(ex[kept])).sum())
    assert bad == 0, "%d of %d elements differ (%s)" % (bad, ex[kept].size, where)
    assert np.array_equal(y[:rows][kept], ey[kept]), where
    # rows past the end of the epoch and rows whose permutation entry lies outside the set keep the sentinel
    assert (bits(x[rows:]) == SENTINEL_X).all() and (y[rows:] == SENTINEL_Y).all(), where
    assert (bits(x[:rows][~kept]) == SENTINEL_X).all() and (y[:rows][~kept] == SENTINEL_Y).all(), where


SIZES = [(12, 8), (40, 36), (72, 64), (256, 224)]


@pytest.mark.parametrize("side,crop", SIZES, ids=["%dto%d" % s for s in SIZES])
def test_kernel_equals_numpy_oracle_bit_for_bit(dev, lut, side, crop):
    """N = 37 at B = 6: seven batches, the last of one row ((rank, world) = (., 2): four global batches, the last of one row on rank
    0 and none on rank 1); both layouts, both pipelines, with and without a permutation - which holds three entries outside the
    set -, advance 0 and world * B."""
    n, B = 37, 6
    images, labels = synthetic(n, side, 100 + side)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).numpy().astype(np.int64)
    perm[3], perm[10], perm[20] = -1, n, 1 << 40
    perm_t = torch.from_numpy(perm).to(dev)
    seed, epoch = 0xDEADBEEF12345678, 6
    n_checked, dropped, offsets = 0, 0, set()
    for train in (True, False):
        ds = device_set(images, labels, crop, train, dev)
        assert (ds.span, ds.off0) == OO.window(side, crop, train) and ds.out_shape == (3, crop, crop)
        assert np.array_equal(bits(ds.lut.cpu().numpy()), bits(lut))
        for with_perm in (True, False):
            for rank, world in ((0, 1), (0, 2), (1, 2)):
                for first in range(0, n, world * B):
                    ex, ey, kept = OO.batch(images, labels, perm if with_perm else None, lut, first, B, rank, world, seed, epoch, crop,
                                            ds.span, ds.off0, ds.flip)
                    assert ex.shape[0] == max(0, min(B, n - (first + rank * B))) and (with_perm or kept.all())
                    dropped += int((~kept).sum())
                    if train:
                        offsets.update(zip(*OO.draws(seed, epoch, first + rank * B + np.arange(ex.shape[0]), ds.span)))
                    for nhwc in (0, 1):
                        for advance in (0, world * B):
                            x, y = launch(dev, ds, perm_t if with_perm else None, epoch, first, B, rank, world, seed, nhwc, advance)
                            check_rows(x, y, ex, ey, kept, "train %s perm %s rank %d/%d first %d nhwc %d advance %d" % (
                                train, with_perm, rank, world, first, nhwc, advance))
                            n_checked += 1
    assert n_checked == 2 * 2 * (7 + 4 + 4) * 4
    assert dropped == 2 * 2 * 3            # the three entries outside the set, once per pipeline and per world size
    # the draws did something: several windows and both orientations occurred
    assert len({o[:2] for o in offsets}) > 10 and {o[2] for o in offsets} == {0, 1}


def test_kernel_batch_of_28_at_256_to_224(dev, lut):
    """The Office shape itself: 28 rows of 224 x 224 from 256 x 256 (784 workgroups), then the short batch of 9"""
    n, B, side, crop = 37, 28, 256, 224
    images, labels = synthetic(n, side, 100 + side)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(8)).numpy().astype(np.int64)
    perm_t = torch.from_numpy(perm).to(dev)
    for train in (True, False):
        ds = device_set(images, labels, crop, train, dev)
        for first in (0, 28):
            ex, ey, kept = OO.batch(images, labels, perm, lut, first, B, 0, 1, 3, 1, crop, ds.span, ds.off0, ds.flip)
            assert ex.shape[0] == (28 if first == 0 else 9)
            for nhwc in (0, 1):
                x, y = launch(dev, ds, perm_t, 1, first, B, 0, 1, 3, nhwc, B)
                check_rows(x, y, ex, ey, kept, "train %s first %d nhwc %d" % (train, first, nhwc))


# ------------------------------------------------------------------------------------------------ the pair loader
SIDE, CROP, NS, NT, B = 72, 64, 20, 15, 6


class PairOracle:
    """The oracle's batches of a PairLoader's iterations: walks data.pair_plan with its own count of passes and positions and reads
    only the loaders' permutations (torch.randperm on the device has no NumPy statement)."""

    def __init__(self, pair, sets, lut):
        from alignq_amd import data as D
        self.pair, self.sets, self.lut = pair, sets, lut
        self.plan = D.pair_plan((NS, B), (NT, B), pair.mode)

    def begin_epoch(self, epoch):
        self.epoch, self.it, self.passes, self.first = epoch, 0, [0, 0], [0, 0]

    def next(self):
        """Call after pair.next_batch_sizes() (a new pass has been begun by then) and before the batch is produced."""
        rows_s, rows_t, new_s, new_t = self.plan[self.it]
        out = []
        for k, (loader, rows, new) in enumerate(((self.pair.src, rows_s, new_s), (self.pair.tgt, rows_t, new_t))):
            if new:
                self.passes[k], self.first[k] = self.passes[k] + 1, 0
            number = self.epoch * (len(self.plan) + 1) + self.passes[k]
            images, labels = self.sets[k]
            assert loader.epoch == number and loader.cursor.cpu().tolist() == [number, self.first[k], 0, 0]
            perm = loader.perm.cpu().numpy()
            assert np.array_equal(np.sort(perm), np.arange(len(images)))
            ds = loader.images
            x, y, kept = OO.batch(images, labels, perm, self.lut, self.first[k], rows, 0, 1, loader.seed, number, ds.crop, ds.span,
                                  ds.off0, ds.flip)
            assert kept.all() and x.shape[0] == rows
            out.append((x, y))
            self.first[k] += rows
        self.it += 1
        return out[0][0], out[0][1], out[1][0], out[1][1]


def make_pair(dev, mode, channels_last=True):
    from alignq_amd import data as D
    sets = [synthetic(NS, SIDE, 51), synthetic(NT, SIDE, 52)]
    src = D.DeviceLoader(device_set(*sets[0], CROP, True, dev), B, seed=11, channels_last=channels_last)
    tgt = D.DeviceLoader(device_set(*sets[1], CROP, True, dev), B, seed=12, channels_last=channels_last)
    return D.PairLoader(src, tgt, mode), sets


@pytest.mark.parametrize("mode", ["zip", "cycle"])
def test_pair_loader_captured_fill_produces_the_oracles_batches(dev, lut, mode):
    """ONE graph holding only pair.record, replayed over two epochs: iteration n of the epoch on the n-th replay, across the passes
    "cycle" begins inside an epoch; the 6 + 3 iteration of "zip" is filled eagerly."""
    pair, sets = make_pair(dev, mode)
    assert len(pair) == (3 if mode == "zip" else 4)
    assert pair.iterations() == ([(6, 6), (6, 6), (6, 3)] if mode == "zip" else [(6, 6)] * 4)
    oracle = PairOracle(pair, sets, lut)
    xs0, ys0, xt0 = pair.peek()
    assert xs0.is_contiguous(memory_format=torch.channels_last) and tuple(xs0.shape) == (B, 3, CROP, CROP) == tuple(xt0.shape)
    sx, sy, sxt = torch.zeros_like(xs0), torch.zeros_like(ys0), torch.zeros_like(xt0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair.record(sx, sy, sxt)
    seen = []
    for epoch in (0, 1):
        pair.begin_epoch(epoch)
        oracle.begin_epoch(epoch)
        for it in range(len(pair)):
            rows = pair.next_batch_sizes()
            assert rows == pair.next_batch_sizes()                         # asking twice begins no second pass
            exs, eys, ext, eyt = oracle.next()
            if rows == (B, B):
                graph.replay()
                pair.skip(*rows)
                xs, ys, xt = sx, sy, sxt
            else:
                assert mode == "zip" and it == 2 and rows == (6, 3)
                xs, ys, xt = pair.next_batch()
            where = (mode, epoch, it)
            assert np.array_equal(bits(xs.cpu().numpy()), bits(exs)) and np.array_equal(ys.cpu().numpy(), eys), where
            assert np.array_equal(bits(xt.cpu().numpy()), bits(ext)), where
            assert np.array_equal(pair.tgt._y[:rows[1]].cpu().numpy(), eyt), where      # the target labels: the loader's own buffer
            seen.append(bits(exs).tobytes())
        assert pair.next_batch_sizes() == (0, 0) and pair.next_batch() is None
    assert len(set(seen)) == len(seen)                                     # no batch repeats: every pass has its own order and draws


def deterministic(on, old=None):
    if on:
        old = (torch.backends.cudnn.deterministic, torch.are_deterministic_algorithms_enabled(),
               torch.is_deterministic_algorithms_warn_only_enabled())
        torch.backends.cudnn.deterministic = True
        torch.use_deterministic_algorithms(True, warn_only=True)
        return old
    torch.backends.cudnn.deterministic = old[0]
    torch.use_deterministic_algorithms(old[1], warn_only=old[2])


def make_step(kind, dev, device_hyper=False):
    from alignq_amd.train_step import DSANTrainStep, OfficeTrainStep
    torch.manual_seed(0)
    net = det_init_(tiny_net(kind, "aligned")).to(dev).train()
    kw = dict(lr=0.004, channels_last=True, fuse_relu=True, dual=True, device_hyper=device_hyper)
    return net, (OfficeTrainStep(net, alpha=0.3, **kw) if kind == "dann" else DSANTrainStep(net, **kw))


@pytest.mark.parametrize("kind,mode", [("dann", "zip"), ("dsan", "cycle")])
def test_office_step_with_pair_in_graph_equals_step_fed_oracle_batches(dev, lut, kind, mode):
    """Twin A: a captured step called with the oracle's batches, step(xs, ys, xt).  Twin B: the same step with set_producer(pair),
    stepped by next().  Twin C: A's sequence once more (the control).  Two epochs of 20 source and 15 target images at batch 6:
    "zip" (DANN) has three iterations, the third of 6 + 3 rows through the eager fallback in every twin; "cycle" (DSAN) four full
    ones with a new target pass at the third and a new source pass at the fourth."""
    from alignq_amd import config, data as D
    old_cfg = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = B
    old_det = deterministic(True)
    try:
        pair, sets = make_pair(dev, mode)
        oracle = PairOracle(pair, sets, lut)
        lambd = {(e, i): 0.1 + 0.2 * e + 0.05 * i for e in (0, 1) for i in range(4)}
        twins = [make_step(kind, dev) for _ in range(3)]
        (net_a, a), (net_b, b), (net_c, c) = twins
        assert b.set_producer(pair) is b
        first = pair.peek()
        for _, step in twins:
            if kind == "dann":
                step.capture(*first, warmup=2)
            else:
                step.capture(*first, warmup=2, lambd=0.05)
            assert step._graph is not None and step._graph2 is None
        with pytest.raises(RuntimeError, match="next"):
            b(*b.static_inputs()) if kind == "dann" else b(*b.static_inputs(), 0.1)
        cu = lambda t: torch.from_numpy(t).to(dev)                         # noqa: E731
        for epoch in (0, 1):
            pair.begin_epoch(epoch)
            oracle.begin_epoch(epoch)
            for it in range(len(pair)):
                rows = pair.next_batch_sizes()
                exs, eys, ext, _ = oracle.next()
                batch = (cu(exs), cu(eys), cu(ext))
                if kind == "dsan":
                    b.set_lambd(lambd[epoch, it])
                graph = b._graph
                ob = b.next()
                assert b._graph is graph
                extra = () if kind == "dann" else (lambd[epoch, it],)
                oa = a(*batch, *extra)
                c(*batch, *extra)
                if rows == (B, B):
                    assert ob is b._outs and oa is a._outs                 # replays
                    got = b.static_inputs()
                    assert np.array_equal(bits(got[0].cpu().numpy()), bits(exs)) and np.array_equal(got[1].cpu().numpy(), eys)
                    assert np.array_equal(bits(got[2].cpu().numpy()), bits(ext))
                else:
                    assert (kind, it, rows) == ("dann", 2, (6, 3)) and ob is not b._outs and oa is not a._outs
                assert torch.isfinite(ob[1]) and torch.isfinite(oa[1])
            with pytest.raises(RuntimeError, match="exhausted"):
                b.next()
        # train_epoch_office drives the same loop (B: replays; A and C: a pair of their own through step(xs, ys, xt))
        if kind == "dsan":
            for _, step in twins:
                step.set_lambd(0.6)
        D.train_epoch_office(b, pair, 2)
        for _, step in ((net_a, a), (net_c, c)):
            own, _ = make_pair(dev, mode)
            D.train_epoch_office(step, own, 2)
        torch.cuda.synchronize()
        st_a, st_b, st_c = (full_state(n_, s_, s_.admms) for n_, s_ in twins)
        bad = differing(st_a, st_c)
        assert not bad, "two runs of the step fed the oracle's batches differ in %d tensors, first: %s" % (len(bad), bad[:6])
        root = "feature." if kind == "dann" else "feature_layers."
        stem = (root + "conv1.", root + "bn1.")
        stem_keys = [k for k in st_a if k.split(":", 1)[1].startswith(stem)]
        assert stem_keys
        for key in stem_keys:
            np.testing.assert_allclose(st_a[key], st_b[key], rtol=1e-5, atol=1e-7 * float(np.abs(st_a[key]).max()) + 1e-12, err_msg=key)
            st_a.pop(key), st_b.pop(key)
        bad = differing(st_a, st_b)
        assert not bad, "the step with the pair in its graph differs from the step fed the oracle's batches in %d tensors, first: %s" % (
            len(bad), bad[:6])
    finally:
        deterministic(False, old_det)
        config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size = old_cfg


def graph_nodes(graph):
    """Number of nodes of a captured torch.cuda.CUDAGraph(keep_graph=True), from the HIP runtime"""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n))
    assert rc == 0, rc
    return int(n.value)


def test_pair_adds_two_nodes_and_an_eval_loader_one(dev, monkeypatch):
    """The producer's launches are all that a graph gains: the tiny DANN's graph with the pair holds exactly two nodes more than
    the graph of a twin step without a producer, a graph holding only pair.record IS two nodes, and the same step with the
    producer detached again captures the twin's count; a DANN EvalStep with a centre-crop loader holds one node more.

    The counts are compared inside one process and not with a recorded number: the tiny network's 17 convolutions (8 .. 64
    channels) run on MIOpen, and how many nodes each of them takes depends on what the process ran before - the producer-less
    graph was counted at 219 nodes when this file ran alone and at 236 when it ran behind the suite's earlier GPU files (17 more:
    one per convolution), with the pair at 221 and 238.  The headline step, whose
    convolutions are the library's own, is held to its recorded 83 nodes by tests/test_gpu_data.py."""
    from alignq_amd import config, data as D
    from alignq_amd.eval_step import EvalStep
    plain = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: plain(keep_graph=True))
    old_cfg = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = B
    try:
        pair, sets = make_pair(dev, "zip")
        first = pair.peek()
        only = torch.cuda.CUDAGraph()
        sx, sy, sxt = (torch.zeros_like(t) for t in first)
        torch.cuda.synchronize()
        with torch.cuda.graph(only):
            pair.record(sx, sy, sxt)
        assert graph_nodes(only) == 2
        counts = []
        for with_pair in (False, True):
            net, step = make_step("dann", dev)
            if with_pair:
                step.set_producer(pair)
            step.capture(*first, warmup=2)
            counts.append(graph_nodes(step._graph))
            if with_pair:
                pair.begin_epoch(0)
                out = step.next()
            else:
                assert step._producer is None
                out = step(*first)
                assert out is step._outs
            torch.cuda.synchronize()
            assert torch.isfinite(out[0]).all() and torch.isfinite(out[1])
        # the producer detached again: the capture is dropped, and the next one is the producer-less graph
        assert step.set_producer(None) is step and step._graph is None
        step.capture(*first, warmup=0)
        counts.append(graph_nodes(step._graph))
        assert step(*first) is step._outs
        torch.cuda.synchronize()
        loader = D.DeviceLoader(device_set(*sets[1], CROP, False, dev), B, channels_last=True)
        ecounts = []
        for with_loader in (False, True):
            ev = EvalStep(net, channels_last=True, qconv=True)
            if with_loader:
                ev.set_producer(loader)
            with ev:
                ev.capture(*loader.peek(), warmup=1)
                ecounts.append(graph_nodes(ev._graph))
        print("graph nodes: train %d / %d with the pair / %d detached again; eval %d / %d with the loader" % (*counts, *ecounts))
        assert counts[1] == counts[0] + 2
        assert counts[2] == counts[0]
        assert ecounts[1] == ecounts[0] + 1
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size = old_cfg


@pytest.mark.parametrize("kind", ["dann", "dsan"])
def test_evaluate_office_test_loader_equals_eval_step_fed_the_oracle(dev, lut, kind):
    """data.evaluate(EvalStep(tiny net), centre-crop loader) - by iteration and with the loader inside the captured graph - equals
    the same EvalStep fed the oracle's tensors: 15 images at batch 6, the last batch of 3; counts identical, the cross-entropy sum
    bit-identical."""
    from alignq_amd import config, data as D
    from alignq_amd.eval_step import EvalStep
    old_cfg = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = B
    try:
        images, labels = synthetic(NT, SIDE, 61)
        ds = device_set(images, labels, CROP, False, dev)
        assert (ds.span, ds.off0) == (1, 4) and not ds.flip and not ds.shuffle
        loader = D.DeviceLoader(ds, B, channels_last=True)
        assert not loader.shuffle and len(loader) == 3
        net, _ = make_step(kind, dev)
        batches = [OO.batch(images, labels, None, lut, k * B, min(B, NT - k * B), 0, 1, 0, 0, CROP, 1, 4, False) for k in range(3)]
        assert [b[0].shape[0] for b in batches] == [6, 6, 3]
        ev = EvalStep(net, channels_last=True, qconv=True)
        with ev:
            for ex, ey, _ in batches:
                ev(torch.from_numpy(ex).to(dev), torch.from_numpy(ey).to(dev))
            expected = ev.counts()
        assert expected[3] == NT and np.isfinite(expected[0])
        with ev:
            got = D.evaluate(ev, loader)
            assert ev.counts() == expected                                 # the ce sum as a double, bit for bit, and the counts
        assert got[3] == NT
        ev.set_producer(loader)
        with ev:
            ev.capture(*loader.peek(), warmup=1)
            D.evaluate(ev, loader)
            assert ev._graph is not None and ev.counts() == expected
        assert net.training and ev._saved is None
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size = old_cfg
