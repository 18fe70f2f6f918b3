"""The pre-packed bf16 filter images: written by the weight quantiser's own launch (alignq_weight_quant_fwd_multi_img), read by the
body and transition convolutions in place of the fp32 filter.  The image element is the expression the fp32 branches evaluate, on
the float the quantiser stores, so everything here is bit for bit: the image against the NumPy statement of the layout
(tests/filter_image_oracle.py) applied to the launch's own q, and every convolution output with an image against without.

Shapes: the body convolutions at their fixed widths with H = 8 and B in {2, 3} (several tiles per image, an image boundary inside the
launch, an odd batch); the transitions at OUTPUT height 8 (input 16 rows: the 1x1 role's tile is 8 output rows) and B = 2."""
import ctypes

import numpy as np
import pytest
import torch

from tests import filter_image_oracle as FO

pytestmark = pytest.mark.gpu

GUARD = 64                    # uint16 elements (128 bytes: the windows stay 16-byte aligned)
GUARD_BITS, PREFILL = 0xA5A5, 0xFFFF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from alignq_amd import _lib
    _lib.load()
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _flip(CO, KK, CI):
    return 1 if (KK == 9 and CO == CI) else 0          # the stride-1 body filters; the transition filters keep the tap order


class Windows:
    """One int16 arena: per image a window pre-filled with 0xFFFF between two guards of 0xA5A5"""

    def __init__(self, dev, sizes):
        self.offs, total = [], 0
        for n in sizes:
            self.offs.append(total + GUARD)
            total += n + 2 * GUARD
        host = np.full(total, GUARD_BITS, dtype=np.uint16)
        for o, n in zip(self.offs, sizes):
            host[o:o + n] = PREFILL
        self.sizes = sizes
        self.buf = torch.from_numpy(host.view(np.int16)).to(dev)
        self.views = [self.buf[o:o + n] for o, n in zip(self.offs, sizes)]
        assert all(v.data_ptr() % 16 == 0 for v in self.views)

    def get(self):
        host = self.buf.cpu().numpy().view(np.uint16)
        imgs = [host[o:o + n].copy() for o, n in zip(self.offs, self.sizes)]
        mask = np.ones(host.size, dtype=bool)
        for o, n in zip(self.offs, self.sizes):
            mask[o:o + n] = False
        return imgs, bool((host[mask] == GUARD_BITS).all())


def _quantise(L, dev, weights, k, formula, geos, with_img):
    """One call of the multi-tensor quantiser over `weights` (flat fp32 tensors); geos[i] = (CO, KK, CI, flip) or None.
    Returns (q, cdf, pdf, ms, windows or None)."""
    lib = L.load()
    T = len(weights)
    q, c, pdf = ([torch.full_like(w, float("nan")) for w in weights] for _ in range(3))
    ms = torch.full((T, 2), float("nan"), device=dev)
    ws = torch.empty(lib.alignq_weight_multi_ws_bytes(T), dtype=torch.uint8, device=dev)
    n = L.i64_array([w.numel() for w in weights])
    win = None
    if with_img:
        sizes = [sum(FO.image_elems(*g[:3])) for g in geos if g is not None]
        for g, s in zip([g for g in geos if g is not None], sizes):
            assert lib.alignq_filter_image_bytes(*g[:3]) == 2 * s
        win = Windows(dev, sizes)
        it = iter(win.views)
        imgs = [None if g is None else next(it) for g in geos]
        geom = []
        for g in geos:
            geom += list(g) if g is not None else [0, 0, 0, 0]
        L.check(lib.alignq_weight_quant_fwd_multi_img(T, L.ptr_array(weights), L.ptr_array(q), L.ptr_array(c), L.ptr_array(pdf), n,
                                                      _p(ms), k, formula, _p(ws), L.ptr_array(imgs),
                                                      (ctypes.c_int32 * len(geom))(*geom), L.stream_ptr()), "fwd_multi_img")
    else:
        L.check(lib.alignq_weight_quant_fwd_multi(T, L.ptr_array(weights), L.ptr_array(q), L.ptr_array(c), L.ptr_array(pdf), n,
                                                  _p(ms), k, formula, _p(ws), L.stream_ptr()), "fwd_multi")
    torch.cuda.synchronize()
    return q, c, pdf, ms, win


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 1. image bits
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("formula", [0, 1])
@pytest.mark.parametrize("form", ["fused", "pair_odd", "pair_large"])
def test_image_bits_equal_the_layout_of_the_launchs_own_q(L, dev, k, formula, form):
    """All seven geometries in one call.  `fused`: the one-launch form.  `pair_*`: one extra tensor WITHOUT an image forces the
    partial + apply pair for the whole call (n % 4 != 0, or more than 36864 elements)."""
    g = torch.Generator().manual_seed(11 * k + formula)
    geos = [(CO, KK, CI, _flip(CO, KK, CI)) for CO, KK, CI in FO.GEOMETRIES]
    weights = [(torch.randn(CO * KK * CI, generator=g) * 0.05).to(dev) for CO, KK, CI, _ in geos]
    if form != "fused":
        weights.append((torch.randn(1001 if form == "pair_odd" else 36868, generator=g) * 0.05).to(dev))
        geos = geos + [None]
    q, c, pdf, ms, win = _quantise(L, dev, weights, k, formula, geos, True)
    q0, c0, pdf0, ms0, _ = _quantise(L, dev, weights, k, formula, geos, False)
    for a, b in zip(q + c + pdf + [ms], q0 + c0 + pdf0 + [ms0]):
        assert _same_bits(a, b)
    imgs, guards_ok = win.get()
    assert guards_ok
    for geo, qi, img in zip([g_ for g_ in geos if g_ is not None], q, imgs):
        want = FO.images(qi.cpu().numpy(), *geo, k)
        assert img.shape == want.shape
        bad = np.flatnonzero(img != want)
        assert bad.size == 0, (geo, bad[:8], img[bad[:8]], want[bad[:8]])


def test_image_arguments_are_validated(L, dev):
    lib = L.load()
    assert lib.alignq_filter_image_bytes(16, 9, 16) == 2 * (5 * 512 + 5 * 512)
    assert lib.alignq_filter_image_bytes(24, 9, 16) == 0 and lib.alignq_filter_image_bytes(16, 0, 16) == 0
    w = torch.randn(16 * 9 * 16, device=dev)
    outs = [torch.empty_like(w) for _ in range(3)]
    ms = torch.empty(1, 2, device=dev)
    ws = torch.empty(lib.alignq_weight_multi_ws_bytes(1), dtype=torch.uint8, device=dev)
    img = torch.empty(5120, dtype=torch.int16, device=dev)

    def call(k, geom):
        return lib.alignq_weight_quant_fwd_multi_img(1, L.ptr_array([w]), L.ptr_array(outs[:1]), L.ptr_array(outs[1:2]),
                                                     L.ptr_array(outs[2:]), L.i64_array([w.numel()]), _p(ms), k, 0, _p(ws),
                                                     L.ptr_array([img]), (ctypes.c_int32 * 4)(*geom), L.stream_ptr())
    assert call(8, (16, 9, 16, 1)) == 0
    assert call(9, (16, 9, 16, 1)) != 0              # bins beyond bf16's 8 significant bits
    assert call(8, (16, 9, 32, 1)) != 0              # geometry does not match n
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- filters with images for 2. / 3.
def _filter(L, dev, CO, KK, CI, k, seed):
    """(q [CO][KK][CI] fp32 on the device, image buffer) from one quantiser launch"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(CO * KK * CI, generator=g) * 0.05).to(dev)
    q, _, _, _, win = _quantise(L, dev, [w], k, 0, [(CO, KK, CI, _flip(CO, KK, CI))], True)
    return q[0], win.views[0]


BODY = [(16, 32, 8), (32, 16, 4), (64, 8, 8)]           # (C, W, w_bit)


def _lazy(dev, g, B, C, HW, form):
    """operands of the lazy batch-norm form: (z, ab, save, ktot, part, dgamma, dbeta)"""
    f32 = dict(dtype=torch.float32, device=dev)
    if form == "plain":
        return (None,) * 7
    z = torch.randn(B * HW * C, generator=g).to(dev)
    ab = (torch.rand(2, C, generator=g) + 0.5).to(dev)
    save = (torch.rand(2, C, generator=g) + 0.5).to(dev)
    if form == "ktot":
        return z, ab, save, (torch.randn(2, C, generator=g) * 0.01).to(dev), None, None, None
    F = C * HW
    tf = 64 if F >= 16384 else 32                  # site_internal.h: bwd_tile_features
    part = (torch.randn(F // tf, min(C, tf), 2, generator=g) * 0.1).to(dev)
    return z, ab, save, None, part, torch.full((C,), float("nan"), **f32), torch.full((C,), float("nan"), **f32)


# ------------------------------------------------------------------------------------------------------- 2. body convolutions
@pytest.mark.parametrize("C,W,k", BODY)
@pytest.mark.parametrize("B", [2, 3])
def test_body_forward_and_data_gradient_with_image_equal_without(L, dev, C, W, k, B):
    lib = L.load()
    H = 8
    q, img = _filter(L, dev, C, 9, C, k, 500 + C)
    g = torch.Generator().manual_seed(600 + C + B)
    st = L.stream_ptr()
    n_parts = lib.alignq_conv3x3_bn_parts(B, H, W, C)
    assert n_parts > 1
    x32 = torch.randn(B, H, W, C, generator=g).to(dev)
    x16 = torch.randint(0, 256, (B, H, W, C), generator=g, dtype=torch.int16).to(dev)
    x8 = torch.randint(0, 16, (B, H, W, C), generator=g, dtype=torch.int8).to(dev)
    for name, x, xb, a_bit in (("fp32", x32, None, 0), ("int16", None, x16, 8), ("int8", None, x8, 4)):
        for with_part in (False, True):
            outs = []
            for use_img in (False, True):
                y = torch.full((B, H, W, C), float("nan"), device=dev)
                part = torch.full((C, n_parts, 2), float("nan"), device=dev) if with_part else None
                tail = (_p(y), B, H, W, C, k, 0, None, _p(part), _p(xb), xb.element_size() if xb is not None else 0, a_bit, st)
                if use_img:
                    L.check(lib.alignq_conv3x3_nhwc_img(_p(x), _p(q), _p(img), *tail), "fwd img")
                else:
                    L.check(lib.alignq_conv3x3_nhwc(_p(x), _p(q), *tail), "fwd")
                outs.append((y, part))
            torch.cuda.synchronize()
            (y0, p0), (y1, p1) = outs
            assert torch.isfinite(y0).all(), name
            assert _same_bits(y0, y1), (name, with_part)
            if with_part:
                assert torch.isfinite(p0).all() and _same_bits(p0, p1), name
    dy = (torch.randn(B, H, W, C, generator=g) * 0.01).to(dev)
    add = torch.randn(B, H, W, C, generator=g).to(dev)
    for a in (None, add):
        dx0, dx1 = (torch.full((B, H, W, C), float("nan"), device=dev) for _ in range(2))
        L.check(lib.alignq_conv3x3_nhwc(_p(dy), _p(q), _p(dx0), B, H, W, C, k, 1, _p(a), None, None, 0, 0, st), "dgrad")
        L.check(lib.alignq_conv3x3_nhwc_img(_p(dy), _p(q), _p(img), _p(dx1), B, H, W, C, k, 1, _p(a), None, None, 0, 0, st), "dgrad img")
        torch.cuda.synchronize()
        assert torch.isfinite(dx0).all() and _same_bits(dx0, dx1), a is not None


@pytest.mark.parametrize("C,W,k", BODY)
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("form", ["plain", "ktot", "part_fill"])
def test_body_one_launch_backward_with_image_equals_without(L, dev, C, W, k, B, form):
    """alignq_conv3x3_nhwc_bwd_fill: dx, the filter-gradient slabs (reduced), the filler role's finished gradient and the published
    batch-norm parameter gradients"""
    lib = L.load()
    H = 8
    q, img = _filter(L, dev, C, 9, C, k, 700 + C)
    g = torch.Generator().manual_seed(800 + C + B)
    st = L.stream_ptr()
    x = torch.randn(B, H, W, C, generator=g).to(dev)
    gy = (torch.randn(B, H, W, C, generator=g) * 0.01).to(dev)
    add = torch.randn(B, H, W, C, generator=g).to(dev)
    nbytes = lib.alignq_conv3x3_wgrad_ws_bytes(C)
    fill = None
    if form == "part_fill":        # an earlier convolution's slabs for the filler role
        ws_f = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ns_f = ctypes.c_int(0)
        L.check(lib.alignq_conv3x3_nhwc_wgrad(_p(x), _p(gy), None, _p(ws_f), B, H, W, C, ctypes.byref(ns_f), None, 0, 0, st), "slabs")
        fill = (ws_f, ns_f.value)
    res = []
    for use_img in (False, True):
        z, ab, save, ktot, part, dgam, dbet = _lazy(dev, torch.Generator().manual_seed(900 + C), B, C, H * W,
                                                    {"plain": "plain", "ktot": "ktot", "part_fill": "part"}[form])
        dx = torch.full((B, H, W, C), float("nan"), device=dev)
        dw = torch.full((C, 9, C), float("nan"), device=dev)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        ns = ctypes.c_int(0)
        fdw = torch.full((C, 9, C), float("nan"), device=dev) if fill else None
        tail = (_p(dx), _p(ws), B, H, W, C, k, ctypes.byref(ns), _p(add), _p(z), _p(ab), _p(save), _p(ktot), _p(part), _p(dgam),
                _p(dbet), None, 0, 0, 1 if fill else 0, L.ptr_array([fill[0]]) if fill else None,
                L.ptr_array([fdw]) if fill else None, (ctypes.c_int * 1)(fill[1]) if fill else None,
                (ctypes.c_int * 1)(9 * C * C) if fill else None, st)
        if use_img:
            L.check(lib.alignq_conv3x3_nhwc_bwd_fill_img(_p(x), _p(gy), _p(q), _p(img), *tail), "bwd_fill img")
        else:
            L.check(lib.alignq_conv3x3_nhwc_bwd_fill(_p(x), _p(gy), _p(q), *tail), "bwd_fill")
        L.check(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws]), L.ptr_array([dw]), (ctypes.c_int * 1)(ns.value),
                                                      (ctypes.c_int * 1)(9 * C * C), st), "reduce")
        torch.cuda.synchronize()
        slabs = ws[:ns.value * 9 * C * C * 4].clone()
        res.append([t for t in (dx, dw, slabs.view(torch.float32), fdw, dgam, dbet) if t is not None])
    assert len(res[0]) == len(res[1]) == 3 + (3 if fill else 0)
    for a, b in zip(*res):
        assert torch.isfinite(a).all()
        assert _same_bits(a, b)


# -------------------------------------------------------------------------------------------------------------- 3. transitions
@pytest.mark.parametrize("CIN,COUT,W,k", [(16, 32, 32, 8), (32, 64, 16, 4)])
def test_transition_forward_and_backward_with_image_equal_without(L, dev, CIN, COUT, W, k):
    lib = L.load()
    B, Hin = 2, 16
    Ho, Wo = Hin // 2, W // 2
    q3, img3 = _filter(L, dev, COUT, 9, CIN, k, 1000 + CIN)
    q1, img1 = _filter(L, dev, COUT, 1, CIN, k, 1001 + CIN)
    g = torch.Generator().manual_seed(1100 + CIN)
    st = L.stream_ptr()
    x = torch.randn(B, Hin, W, CIN, generator=g).to(dev)
    np3 = lib.alignq_conv_gen_bn_parts(B, Hin, W, CIN, COUT, 3, 2)
    np1 = lib.alignq_conv_gen_bn_parts(B, Hin, W, CIN, COUT, 1, 2)
    assert np3 > 1 and np1 > 1

    def nan(*shape):
        return torch.full(shape, float("nan"), device=dev)
    # forward: both roles, stand-alone and in one launch
    res = []
    for use_img in (False, True):
        y3, y1, z3, z1 = (nan(B, Ho, Wo, COUT) for _ in range(4))
        p3, p1, r3, r1 = nan(COUT, np3, 2), nan(COUT, np1, 2), nan(COUT, np3, 2), nan(COUT, np1, 2)
        t3 = (_p(y3), B, Hin, W, CIN, COUT, 3, 2, k, _p(p3), st)
        t1 = (_p(y1), B, Hin, W, CIN, COUT, 1, 2, k, _p(p1), st)
        tt = (_p(z3), _p(z1), B, Hin, W, CIN, COUT, k, _p(r3), _p(r1), st)
        if use_img:
            L.check(lib.alignq_conv_gen_nhwc_fwd_img(_p(x), _p(q3), _p(img3), *t3), "fwd 3x3 img")
            L.check(lib.alignq_conv_gen_nhwc_fwd_img(_p(x), _p(q1), _p(img1), *t1), "fwd 1x1 img")
            L.check(lib.alignq_transition_nhwc_fwd_img(_p(x), _p(q3), _p(q1), _p(img3), _p(img1), *tt), "transition fwd img")
        else:
            L.check(lib.alignq_conv_gen_nhwc_fwd(_p(x), _p(q3), *t3), "fwd 3x3")
            L.check(lib.alignq_conv_gen_nhwc_fwd(_p(x), _p(q1), *t1), "fwd 1x1")
            L.check(lib.alignq_transition_nhwc_fwd(_p(x), _p(q3), _p(q1), *tt), "transition fwd")
        torch.cuda.synchronize()
        res.append([y3, y1, z3, z1, p3, p1, r3, r1])
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and _same_bits(a, b)
    # backward: the stand-alone data gradients (plain, with add) and the one-launch backward (lazy batch-norm records, publishing)
    gy3 = (torch.randn(B, Ho, Wo, COUT, generator=g) * 0.01).to(dev)
    gy1 = (torch.randn(B, Ho, Wo, COUT, generator=g) * 0.01).to(dev)
    add = torch.randn(B, Hin, W, CIN, generator=g).to(dev)
    res = []
    for use_img in (False, True):
        out = []
        for ks, qf, im, gy in ((3, q3, img3, gy3), (1, q1, img1, gy1)):
            for a in (None, add):
                dx = nan(B, Hin, W, CIN)
                tail = (_p(dx), B, Hin, W, CIN, COUT, ks, 2, k, _p(a), None, None, None, None, None, None, None, st)
                if use_img:
                    L.check(lib.alignq_conv_gen_nhwc_dgrad_img(_p(gy), _p(qf), _p(im), *tail), "dgrad img")
                else:
                    L.check(lib.alignq_conv_gen_nhwc_dgrad(_p(gy), _p(qf), *tail), "dgrad")
                out.append(dx)
        for form in ("plain", "ktot", "part"):
            l3 = _lazy(dev, torch.Generator().manual_seed(1200 + CIN), B, COUT, Ho * Wo, form)
            l1 = _lazy(dev, torch.Generator().manual_seed(1300 + CIN), B, COUT, Ho * Wo, form)
            dx = nan(B, Hin, W, CIN)
            dw3, dw1 = nan(COUT, 9, CIN), nan(COUT, 1, CIN)
            ws3 = torch.zeros(lib.alignq_conv_gen_wgrad_ws_bytes(CIN, COUT, 3), dtype=torch.uint8, device=dev)
            ws1 = torch.zeros(lib.alignq_conv_gen_wgrad_ws_bytes(CIN, COUT, 1), dtype=torch.uint8, device=dev)
            ns3, ns1 = ctypes.c_int(0), ctypes.c_int(0)
            tail = (_p(dx), _p(ws3), _p(ws1), B, Hin, W, CIN, COUT, k, ctypes.byref(ns3), ctypes.byref(ns1), None,
                    *[_p(t) for t in l3], *[_p(t) for t in l1], st)
            if use_img:
                L.check(lib.alignq_transition_nhwc_bwd_img(_p(x), _p(gy3), _p(gy1), _p(q3), _p(q1), _p(img3), _p(img1), *tail),
                        "transition bwd img")
            else:
                L.check(lib.alignq_transition_nhwc_bwd(_p(x), _p(gy3), _p(gy1), _p(q3), _p(q1), *tail), "transition bwd")
            L.check(lib.alignq_conv3x3_wgrad_reduce_multi(
                2, L.ptr_array([ws3, ws1]), L.ptr_array([dw3, dw1]), (ctypes.c_int * 2)(ns3.value, ns1.value),
                (ctypes.c_int * 2)(9 * CIN * COUT, CIN * COUT), st), "reduce")
            torch.cuda.synchronize()
            out += [dx, dw3, dw1, ws3[:ns3.value * 9 * CIN * COUT * 4].clone().view(torch.float32),
                    ws1[:ns1.value * CIN * COUT * 4].clone().view(torch.float32)]
            out += [t for t in (l3[5], l3[6], l1[5], l1[6]) if t is not None]
        res.append(out)
    assert len(res[0]) == len(res[1]) == 4 + 3 * 5 + 4
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and _same_bits(a, b)


# --------------------------------------------------------------------------------------------------------------- 4. whole step
def graph_nodes(graph):
    """Number of nodes of a captured torch.cuda.CUDAGraph(keep_graph=True), from the HIP runtime"""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n))
    assert rc == 0, rc
    return int(n.value)


def test_resnet20_step_with_images_equals_without(dev, monkeypatch):
    """Two ResNet-20 twins (8W/8A, CDF + ADMM, batch 128, channels-last), filter images on and off: two eager steps, capture, two
    replays; every parameter, momentum buffer and output bit-equal; the captured graphs hold the same number of nodes."""
    from alignq_amd import config, fused
    from alignq_amd.resnet import resnet20_quant
    from alignq_amd.train_step import TrainStep
    plain = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: plain(keep_graph=True))
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size)
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    try:
        g = torch.Generator().manual_seed(3)
        xs = [torch.randn(128, 3, 32, 32, generator=g).to(dev) for _ in range(4)]
        ys = [torch.randint(0, 10, (128,), generator=g).to(dev) for _ in range(4)]
        runs = []
        for on in (True, False):
            torch.manual_seed(7)
            model = resnet20_quant(8, 8).to(dev).train()
            step = TrainStep(model, channels_last=True, qconv=True, filter_images=on)
            assert step.filter_images is on
            outs = [tuple(t.clone() for t in step(xs[i], ys[i])) for i in range(2)]
            with_img = [c for c in step.all_convs if fused.filter_image_geometry(c.weight) is not None]
            assert len(with_img) == 20               # every convolution but the stem
            step.capture(xs[2], ys[2], warmup=0)
            nodes = graph_nodes(step._graph)
            for i in (2, 3):
                outs.append(tuple(t.clone() for t in step(xs[i], ys[i])))
            torch.cuda.synchronize()
            state = {n: p.detach().clone() for n, p in model.named_parameters()}
            for n, p in model.named_parameters():
                buf = step.optimizer_t.state.get(p, {}).get("momentum_buffer")
                if buf is not None:
                    state["momentum." + n] = buf.detach().clone()
            runs.append((outs, state, nodes))
        (o1, s1, n1), (o0, s0, n0) = runs
        print("graph nodes: %d with filter images, %d without" % (n1, n0))
        assert n1 == n0
        for a, b in zip(o1, o0):
            for t, u in zip(a, b):
                assert torch.isfinite(t).all() and _same_bits(t.float().contiguous(), u.float().contiguous())
        assert s1.keys() == s0.keys() and any(k_.startswith("momentum.") for k_ in s1)
        bad = [k_ for k_ in s1 if not _same_bits(s1[k_].contiguous(), s0[k_].contiguous())]
        assert not bad, bad[:6]
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size = old


# --------------------------------------------------------------------------------------------------------------- 5. evaluation
def test_eval_step_with_images_equals_without_and_builds_them_once(dev, monkeypatch):
    from alignq_amd import config, fused
    from alignq_amd.eval_step import EvalStep
    from alignq_amd.resnet import resnet20_quant
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = 100
    calls = []
    real = fused.prequantize_weights
    monkeypatch.setattr(fused, "prequantize_weights", lambda *a, **kw: (calls.append(kw.get("images")), real(*a, **kw))[1])
    try:
        g = torch.Generator().manual_seed(5)
        xs = [torch.randn(100, 3, 32, 32, generator=g).to(dev) for _ in range(2)]
        ys = [torch.randint(0, 10, (100,), generator=g).to(dev) for _ in range(2)]
        torch.manual_seed(9)
        model = resnet20_quant(8, 8).to(dev)
        logits = {}
        for on in (True, False):
            del calls[:]
            ev = EvalStep(model, channels_last=True, qconv=True, filter_images=on)
            with ev:
                held = {id(c.quantize_fn): c.quantize_fn.parked.image for c in ev.all_convs
                        if c.quantize_fn.parked is not None and c.quantize_fn.parked.image is not None}
                assert len(held) == (20 if on else 0)
                used = []            # (quantiser, image) of every image a convolution was handed for its kernel
                qcls = type(ev.all_convs[1].quantize_fn)
                real_filter_of = qcls.filter_of

                def spy(self, wq):
                    rec = real_filter_of(self, wq)
                    if rec.image is not None:
                        used.append((id(self), rec.image))
                    return rec
                monkeypatch.setattr(qcls, "filter_of", spy)
                logits[on] = [ev(x, y).clone() for x, y in zip(xs, ys)]
                monkeypatch.setattr(qcls, "filter_of", real_filter_of)
                # both batches read the buffers the one quantiser launch of begin() wrote: each of the 20 convolutions once per batch
                assert calls == [on]
                assert len(used) == (2 * 20 if on else 0)
                if on:
                    assert sorted(q for q, _ in used) == sorted(2 * list(held))
                    assert {im.data_ptr() for _, im in used} == {h.data_ptr() for h in held.values()}
            torch.cuda.synchronize()
        for a, b in zip(logits[True], logits[False]):
            assert torch.isfinite(a).all() and _same_bits(a.contiguous(), b.contiguous())
    finally:
        (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size) = old
