"""The depthwise 3x3 kernels (csrc/dwconv_kernels.hip) against tests/dwconv_oracle.py: forward and data gradient bit for bit against the
float32 statement, the filter gradient within gamma_{N+1} * sum |x * dy| of float64, every launch twice (same bits), every output
written into a NaN-filled window between sentinel guards.  Then the refusals, ops.QConvDwFn through autograd, Conv2d_Q's dispatch and
a captured chain of the three launches.  Reference op: Conv2d_Q.forward's F.conv2d at groups == channels
(cdf_alignment/mobilenet-v2-svhn/model/mobilenetV2.py:40, model/quantization.py:116-120)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_oracle as D

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC05A5A         # a quiet NaN no kernel here produces
GUARD = 64
ACT_RANGE = 2.0

# (B, C, H, W), each at stride 1 and 2
SHAPES = [
    (2, 4, 1, 1),           # every tap but the centre is padding
    (3, 20, 5, 7),          # odd, non-square, C neither a power of two nor a multiple of 8
    (3, 20, 6, 8),          # even sizes
    (2, 144, 9, 9),         # a MobileNet channel count on an odd map
    (4, 960, 4, 4),         # C far above a workgroup's lanes on a tiny map
    (8, 96, 32, 32),        # many filter-gradient slabs
    (8, 144, 32, 32),       # beyond one pass of the capped grid (1152 workgroups' worth; the stride keeps every thread on its quad)
    (1, 8212, 12, 12),      # beyond one pass AND no grid stride that is a multiple of the 2053 quads: filters reloaded per item
]
CASES = [(shape, s) for shape in SHAPES for s in (1, 2)]
FP32_FILTER_CASE = ((3, 20, 5, 7), 2)       # the one case with an unquantised filter


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Arena:
    """16-byte aligned windows of the given sizes in one sentinel-filled device buffer, GUARD elements apart"""

    def __init__(self, dev, sizes):
        self.offs, off = [], 0
        for n in sizes:
            off = (off + GUARD + 3) // 4 * 4
            self.offs.append(off)
            off += n
        self.sizes, self.total = list(sizes), off + GUARD
        self.inside = np.zeros(self.total, bool)
        for o, n in zip(self.offs, self.sizes):
            self.inside[o:o + n] = True
        self.buf = torch.full((self.total,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + n] for o, n in zip(self.offs, self.sizes)]

    def reset(self):
        self.buf.view(torch.int32).fill_(SENTINEL)

    def raw(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def get(self):
        """the windows' contents; asserts that everything outside them still holds the sentinel bit for bit"""
        host = self.buf.cpu().numpy()
        assert np.all(host.view(np.uint32)[~self.inside] == SENTINEL), "a kernel wrote outside its tensor"
        return [host[o:o + n].copy() for o, n in zip(self.offs, self.sizes)]


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def nchw(flat, B, C, H, W):
    return np.ascontiguousarray(flat.reshape(B, H, W, C).transpose(0, 3, 1, 2))


def levels_relu(rng, shape):
    """what the layers really see: relu(4-bit levels * act_range), with many exact zeros"""
    lv = (2.0 * rng.integers(0, 16, shape) / 15.0 - 1.0) * ACT_RANGE
    return np.maximum(lv, 0.0).astype(np.float32)


def make_case(shape, s, idx):
    B, C, H, W = shape
    rng = np.random.default_rng(1900 + idx)
    Ho, Wo = D.out_size(H, s), D.out_size(W, s)
    if idx % 2:
        x, dy = levels_relu(rng, shape), levels_relu(rng, (B, C, Ho, Wo))
    else:
        x, dy = rng.standard_normal(shape).astype(np.float32), rng.standard_normal((B, C, Ho, Wo)).astype(np.float32)
    if (shape, s) == FP32_FILTER_CASE:
        w = (rng.standard_normal((C, 1, 3, 3)) * 0.3).astype(np.float32)
    else:
        w = (2.0 * rng.integers(0, 16, (C, 1, 3, 3)) / 15.0 - 1.0).astype(np.float32)      # W_q's 4-bit level values
    return x, w, dy


class Launch:
    """the three launches on one shape, outputs in an arena"""

    def __init__(self, dev, shape, s):
        from alignq_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.B, self.C, self.H, self.W = shape
        self.s, self.dev = s, dev
        self.Ho, self.Wo = D.out_size(self.H, s), D.out_size(self.W, s)
        self.arena = Arena(dev, [self.B * self.Ho * self.Wo * self.C, self.B * self.H * self.W * self.C, self.C * 9])
        self.ws = torch.empty(max(int(self.lib.alignq_dwconv3x3_wgrad_ws_bytes(self.B, self.H, self.W, self.C, s)), 256),
                              dtype=torch.uint8, device=dev)

    def args(self):
        return (self.B, self.H, self.W, self.C, self.s, self.L.stream_ptr())

    def run(self, x, w, dy, which=("fwd", "dgrad", "wgrad")):
        """x, w, dy: device tensors (flat NHWC / [C * 9]); returns the return codes"""
        y, dx, dw = self.arena.views
        rc = {}
        if "fwd" in which:
            rc["fwd"] = self.lib.alignq_dwconv3x3_nhwc_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), *self.args())
        if "dgrad" in which:
            rc["dgrad"] = self.lib.alignq_dwconv3x3_nhwc_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), *self.args())
        if "wgrad" in which:
            rc["wgrad"] = self.lib.alignq_dwconv3x3_nhwc_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), self.ws.data_ptr(),
                                                                *self.args())
        torch.cuda.synchronize()
        return rc

    def results(self):
        y, dx, dw = self.arena.get()
        return (nchw(y, self.B, self.C, self.Ho, self.Wo), nchw(dx, self.B, self.C, self.H, self.W), dw.reshape(self.C, 3, 3))


def to_dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev) for a in arrays]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-s{c[1]}" for c in CASES])
def test_three_launches_against_the_oracle(dev, idx):
    shape, s = CASES[idx]
    B, C, H, W = shape
    x, w, dy = make_case(shape, s, idx)
    run = Launch(dev, shape, s)
    xd, wd, dyd = to_dev(dev, nhwc(x), w, nhwc(dy))
    assert all(v == 0 for v in run.run(xd, wd, dyd).values())
    y, dx, dw = run.results()
    assert not np.isnan(y).any() and not np.isnan(dx).any() and not np.isnan(dw).any()      # every element of the windows was written
    y32, dx32 = D.fwd32(x, w, s), D.dgrad32(dy, w, s, H, W)
    ny, nx = int((y.view(np.uint32) != y32.view(np.uint32)).sum()), int((dx.view(np.uint32) != dx32.view(np.uint32)).sum())
    err = np.abs(dw - D.wgrad64(x, dy, s))
    bound = D.wgrad_bound(x, dy, s)
    print(f"{shape} s{s}: y bits differ {ny}, dx bits differ {nx}, dw max err {err.max():.3e}, "
          f"max err / bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert ny == 0, "forward is not bit-equal to the float32 statement"
    assert nx == 0, "data gradient is not bit-equal to the float32 statement"
    assert (err <= bound).all()
    if s == 2:       # input positions no output reads: exactly +0
        never = D.dgrad_mag(np.ones_like(dy), np.ones_like(w), s, H, W) == 0
        assert (dx.view(np.uint32)[never] == 0).all()
    # a second launch into fresh NaN windows: the same bits
    run.arena.reset()
    assert all(v == 0 for v in run.run(xd, wd, dyd).values())
    y2, dx2, dw2 = run.results()
    assert D.bits_equal(y, y2) and D.bits_equal(dx, dx2) and D.bits_equal(dw, dw2)


@pytest.mark.parametrize("C,s", [(6, 1), (8, 3)])
def test_refusals_leave_the_windows_untouched(dev, C, s):
    from alignq_amd import _lib as L
    shape = (2, C, 6, 6)
    run = Launch(dev, shape, s if s in (1, 2) else 1)
    run.s = s
    xd, wd, dyd = to_dev(dev, np.ones((2, 6, 6, C), np.float32), np.ones((C, 9), np.float32), np.ones((2, 6, 6, C), np.float32))
    rc = run.run(xd, wd, dyd)
    assert rc == {"fwd": L.EUNSUPPORTED, "dgrad": L.EUNSUPPORTED, "wgrad": L.EUNSUPPORTED}
    assert (run.arena.raw() == SENTINEL).all()
    assert L.load().alignq_dwconv3x3_supported(2, 6, 6, C, s) == 0


def _count(monkeypatch, lib, names):
    calls = {n: 0 for n in names}
    for n in names:
        orig = getattr(lib, n)

        def wrapper(*a, _n=n, _orig=orig):
            calls[_n] += 1
            return _orig(*a)
        monkeypatch.setattr(lib, n, wrapper)
    return calls


LAUNCHES = ("alignq_dwconv3x3_nhwc_fwd", "alignq_dwconv3x3_nhwc_dgrad", "alignq_dwconv3x3_nhwc_wgrad")


@pytest.mark.parametrize("s", [1, 2])
def test_autograd_path_equals_the_direct_launches(dev, monkeypatch, s):
    from alignq_amd import _lib as L
    from alignq_amd import ops
    shape = (3, 20, 5, 7)
    B, C, H, W = shape
    x, w, dy = make_case(shape, s, 100 + s)
    run = Launch(dev, shape, s)
    xd, wd, dyd = to_dev(dev, nhwc(x), w, nhwc(dy))
    assert all(v == 0 for v in run.run(xd, wd, dyd).values())
    y0, dx0, dw0 = run.results()
    cl = torch.channels_last
    xt = torch.from_numpy(x).to(dev).contiguous(memory_format=cl)
    wt = torch.from_numpy(w).to(dev)
    gy = torch.from_numpy(dy).to(dev)                   # NCHW-contiguous: backward makes it channels-last
    calls = _count(monkeypatch, L.load(), LAUNCHES)
    for need_x, need_w in ((True, True), (True, False), (False, True)):
        for k in calls:
            calls[k] = 0
        xi, wi = xt.clone(memory_format=cl).requires_grad_(need_x), wt.clone().requires_grad_(need_w)
        y = ops.QConvDwFn.apply(xi, wi, s)
        assert y.is_contiguous(memory_format=cl) and tuple(y.shape) == (B, C, D.out_size(H, s), D.out_size(W, s))
        y.backward(gy)
        torch.cuda.synchronize()
        assert calls == {LAUNCHES[0]: 1, LAUNCHES[1]: int(need_x), LAUNCHES[2]: int(need_w)}
        assert D.bits_equal(y.detach().cpu().numpy(), y0)
        if need_x:
            assert xi.grad.stride() == xi.stride() and D.bits_equal(xi.grad.cpu().numpy(), dx0)
        else:
            assert xi.grad is None
        if need_w:
            assert wi.grad.shape == wi.shape and wi.grad.stride() == wi.stride()
            assert D.bits_equal(wi.grad.cpu().numpy().reshape(C, 3, 3), dw0)
        else:
            assert wi.grad is None


def test_conv2d_q_dispatch(dev, monkeypatch):
    import alignq_amd.cdf_alignment as A
    from alignq_amd import _lib as L
    calls = _count(monkeypatch, L.load(), LAUNCHES)
    cl = torch.channels_last
    C, s = 20, 2
    torch.manual_seed(3)
    conv = A.conv2d_Q_fn(4, "no_align")(C, C, 3, s, 1, groups=C, bias=False).to(dev)
    x = torch.randn(3, C, 6, 8, device=dev)
    xcl = x.contiguous(memory_format=cl)
    wq = conv.quantize_fn(conv.weight).detach()
    want = F.conv2d(x, wq, None, s, 1, 1, C)
    bound = torch.from_numpy(2 * D.fwd_bound(x.cpu().numpy(), wq.cpu().numpy(), s)).to(dev)

    assert (conv(xcl) - want).abs().le(bound).all() and calls[LAUNCHES[0]] == 0          # use_qconv not set: F.conv2d as before
    conv.use_qconv = True
    assert (conv(x) - want).abs().le(bound).all() and calls[LAUNCHES[0]] == 0            # NCHW input: F.conv2d as before
    y = conv(xcl)
    assert calls[LAUNCHES[0]] == 1 and y.is_contiguous(memory_format=cl)
    assert D.bits_equal(y.detach().cpu().numpy(), D.fwd32(x.cpu().numpy(), wq.cpu().numpy(), s))
    y.sum().backward()                                                                   # the filter gradient reaches the raw filter
    assert calls[LAUNCHES[2]] == 1 and calls[LAUNCHES[1]] == 0 and torch.isfinite(conv.weight.grad).all()

    dense = A.conv2d_Q_fn(4, "no_align")(8, 8, 3, 1, 1, bias=False).to(dev).to(memory_format=cl)
    dense.use_qconv = True
    before = dict(calls)
    dense(torch.randn(2, 8, 6, 6, device=dev).contiguous(memory_format=cl))
    assert calls == before                                                               # groups == 1 never reaches the depthwise kernels


def test_captured_chain_replays_to_the_eager_bits(dev):
    shape, s = (3, 20, 6, 8), 2
    x, w, dy = make_case(shape, s, 200)
    run = Launch(dev, shape, s)                          # arena and workspace exist before the capture
    xd, wd, dyd = to_dev(dev, nhwc(x), w, nhwc(dy))
    assert all(v == 0 for v in run.run(xd, wd, dyd).values())
    eager = run.results()
    run.arena.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):           # one stream: forward -> data gradient -> filter gradient (two kernels), a chain
        y, dx, dw = run.arena.views
        a = (run.B, run.H, run.W, run.C, s, run.L.stream_ptr())
        assert run.L.stream_ptr() == side.cuda_stream
        rcs = [run.lib.alignq_dwconv3x3_nhwc_fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), *a),
               run.lib.alignq_dwconv3x3_nhwc_dgrad(dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), *a),
               run.lib.alignq_dwconv3x3_nhwc_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), run.ws.data_ptr(), *a)]
    assert rcs == [0, 0, 0]
    for _ in range(2):
        run.arena.reset()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(run.results(), eager):
            assert D.bits_equal(got, want)
