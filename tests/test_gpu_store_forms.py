"""The write-through output stores (csrc/store_forms.h) of the batch-128 site kernels and the CIFAR convolutions at their smallest
legal shapes: every output element is written, nothing outside the output is touched (outputs live inside sentinel-filled buffers),
forms of the same arithmetic that keep plain stores (the masked one-tile site forward, the dword site backward) or take another
launch path (twin / two launches, one-launch backward / stand-alone gradients) give the same bits, and a captured producer ->
consumer pair replays to the bits of the eager run."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1024                      # elements on each side of an output
SENT = 0x7FC0DEAD                 # a NaN pattern no kernel produces
K, B128 = 8, 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from alignq_amd import _lib as L
    return L.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _check(rc, what):
    from alignq_amd import _lib as L
    L.check(rc, what)


class Guarded:
    """n elements of `dtype` (4 or 2 bytes) inside a sentinel-filled buffer, `shift` elements past a 16-byte boundary"""

    def __init__(self, dev, n, dtype=torch.float32, shift=0):
        self.n, self.dtype, self.lo = n, dtype, GUARD + shift
        it = torch.int32 if dtype == torch.float32 else torch.int16
        self.sent = SENT if it == torch.int32 else 0x7EAD
        self.raw = torch.full((n + 2 * GUARD + 8,), self.sent, dtype=it, device=dev)
        self.out = self.raw[self.lo:self.lo + n].view(dtype)

    def assert_written_and_bands_intact(self, what, n_written=None):
        raw = self.raw.cpu().numpy()
        n = self.n if n_written is None else n_written
        assert (raw[:self.lo] == self.sent).all() and (raw[self.lo + self.n:] == self.sent).all(), what + ": a guard band changed"
        body = raw[self.lo:self.lo + n]
        assert (body != self.sent).all(), (what, "elements not written", int((body == self.sent).sum()))


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ the sites
C_S, H_S = 16, 8
HW_S, F_S = H_S * H_S, C_S * H_S * H_S


class SiteCase:
    def __init__(self, dev, seed):
        g = torch.Generator().manual_seed(seed)
        self.z = (torch.randn(B128, F_S, generator=g) * 1.5 + 0.2).to(dev)
        self.res = torch.randn(B128, F_S, generator=g).to(dev)
        self.gy = (torch.randn(B128, F_S, generator=g) * 1e-2).to(dev)
        self.gam = (torch.rand(C_S, generator=g) + 0.5).to(dev)
        self.bet = (torch.randn(C_S, generator=g) * 0.2).to(dev)
        self.A = (torch.randn(128, 128, generator=g) * 0.05).to(dev)
        self.Gm = (torch.randn(128, 128, generator=g) * 0.05).to(dev)


def _site_fwd_args(lib, dev, c, relu, use_res, want_bins, shift=0):
    from alignq_amd import _lib as L
    f32 = dict(dtype=torch.float32, device=dev)
    part = torch.empty(lib.alignq_bn_nhwc_ws_bytes(C_S), dtype=torch.uint8, device=dev)
    _check(lib.alignq_bn_partial_stats_nhwc(_p(c.z), B128, C_S, HW_S, _p(part), None), "bn_partial_stats_nhwc")
    n_ws = lib.alignq_site_ws_bytes(B128, F_S) // 4
    t = dict(part=part, ab=torch.empty(2, C_S, **f32), save=torch.empty(2, C_S, **f32), rm=torch.zeros(C_S, **f32),
             rv=torch.ones(C_S, **f32), nbt=torch.zeros((), dtype=torch.int64, device=dev), stats=torch.empty(4, F_S, **f32),
             ws=Guarded(dev, n_ws), y=Guarded(dev, B128 * F_S, shift=shift),
             bins=Guarded(dev, B128 * F_S, torch.int16) if want_bins else None)
    t["ws"].out[_site_slab_floats(lib):] = 0           # the reduction tail behind the slabs (loss partials, ticket) starts zeroed
    a = L.SiteBnArgs(_p(c.z), _p(part), _p(c.gam), _p(c.bet), _p(t["rm"]), _p(t["rv"]), _p(t["nbt"]), 0.1, 1e-5, _p(t["ab"]),
                     _p(t["save"]), C_S, HW_S, B128, F_S, K, 2.0, 0.0, int(relu), _p(c.res) if use_res else None, 1, 0,
                     _p(t["y"].out), _p(t["bins"].out) if want_bins else None, _p(t["stats"]), _p(t["ws"].out))
    return a, t


def _launch_fwd(lib, a):
    _check(lib.alignq_site_partials_bn(a.z, a.bn_part, a.bn_gamma, a.bn_beta, a.running_mean, a.running_var, a.num_batches_tracked,
                                       a.momentum, a.bn_eps, a.ab, a.save, a.C, a.HW, a.B, a.F, a.k, a.act_range, a.eps, a.relu,
                                       a.residual, a.nhwc, a.conv_parts, a.xq, a.bins_out, a.stats, a.ws, None), "site_partials_bn")


def _site_slab_floats(lib):
    n_tiles = F_S // 32                            # 32-feature tiles at F <= 4096 (site_internal.h: geom)
    return n_tiles * 8256                          # kSlab4Floats per workgroup


def _fwd_outputs(t, lib):
    out = dict(y=_bits(t["y"].out), stats=_bits(t["stats"]), ab=_bits(t["ab"]), save=_bits(t["save"]),
               slabs=_bits(t["ws"].out[:_site_slab_floats(lib)]))
    if t["bins"] is not None:
        out["bins"] = _bits(t["bins"].out)
    return out


def _assert_fwd_guards(t, lib, what):
    t["y"].assert_written_and_bands_intact(what + " y")
    t["ws"].assert_written_and_bands_intact(what + " slabs", _site_slab_floats(lib))
    if t["bins"] is not None:
        t["bins"].assert_written_and_bands_intact(what + " bins")


@pytest.mark.parametrize("use_res,want_bins", [(True, False), (False, True), (False, False)])
def test_site_forward_outputs_guards_and_launch_forms(dev, lib, use_res, want_bins):
    """The one-tile forward at B = 128, F = 1024 (32 tiles of 32 features): complete-tile form (write-through x_q / y and slabs), the
    masked form (x_q four bytes off a 16-byte boundary: plain scalar stores) and the twin launch: same bits, every element
    written, guard bands intact."""
    c, c2 = SiteCase(dev, 11), SiteCase(dev, 12)
    relu = True
    a, t = _site_fwd_args(lib, dev, c, relu, use_res, want_bins)
    _launch_fwd(lib, a)
    torch.cuda.synchronize()
    _assert_fwd_guards(t, lib, "single")
    ref = _fwd_outputs(t, lib)
    assert np.isfinite(t["y"].out.cpu().numpy()).all()
    if not want_bins:                                            # (the index output needs the aligned form)
        am, tm = _site_fwd_args(lib, dev, c, relu, use_res, False, shift=1)
        _launch_fwd(lib, am)
        torch.cuda.synchronize()
        _assert_fwd_guards(tm, lib, "masked")
        got = _fwd_outputs(tm, lib)
        for key in ref:
            assert np.array_equal(ref[key], got[key]), ("masked form", key)
    # twin: this site and a second one in one launch against their single launches
    a1, t1 = _site_fwd_args(lib, dev, c, relu, use_res, want_bins)
    a2, t2 = _site_fwd_args(lib, dev, c2, False, False, False)
    _check(lib.alignq_site_partials_bn_twin(ctypes.byref(a1), ctypes.byref(a2), None), "twin")
    b2, u2 = _site_fwd_args(lib, dev, c2, False, False, False)
    _launch_fwd(lib, b2)
    torch.cuda.synchronize()
    for tt, what in ((t1, "twin a"), (t2, "twin b")):
        _assert_fwd_guards(tt, lib, what)
    for got, want, what in ((_fwd_outputs(t1, lib), ref, "twin a"), (_fwd_outputs(t2, lib), _fwd_outputs(u2, lib), "twin b")):
        for key in want:
            assert np.array_equal(want[key], got[key]), (what, key)


def _site_bwd_setup(lib, dev, c, use_res, want_bins):
    """forward of one site, then S from the reduction + preparation entry points"""
    a, t = _site_fwd_args(lib, dev, c, True, use_res, want_bins)
    _launch_fwd(lib, a)
    D, scal = torch.empty(B128, B128, device=dev), torch.empty(4, device=dev)
    _check(lib.alignq_site_reduce_loss(_p(t["ws"].out), B128, F_S, _p(D), _p(c.A), _p(c.Gm), 128, 0.2, 0.3, _p(scal), None), "reduce")
    S = torch.zeros(lib.alignq_site_bwd_ws_bytes(B128) // 4, device=dev)
    one, dA, dG = torch.ones((), device=dev), torch.empty_like(c.A), torch.empty_like(c.Gm)
    _check(lib.alignq_site_prep_fused(_p(D), _p(c.A), _p(c.Gm), 128, _p(scal), 0.2, _p(one), B128, F_S, _p(S), _p(dA), _p(dG), None), "prep")
    return t, S


def _site_bwd_args(lib, dev, c, t, S, use_res, want_bins, shift=0):
    from alignq_amd import _lib as L
    o = dict(dx=Guarded(dev, B128 * F_S, shift=shift), dres=Guarded(dev, B128 * F_S) if use_res else None,
             part=torch.zeros(lib.alignq_site_bn_part_bytes(F_S, 1), dtype=torch.uint8, device=dev))
    q = L.SiteBwdBnArgs(_p(c.gy), _p(S), _p(c.z), _p(t["ab"]), _p(t["save"]), C_S, HW_S, 1, None if want_bins else _p(t["y"].out),
                        _p(t["bins"].out) if want_bins else None, 2 if want_bins else 0, _p(o["dres"].out) if use_res else None,
                        _p(t["stats"]), B128, F_S, 2.0, 0.0, _p(o["dx"].out), _p(o["part"]))
    return q, o


def _launch_bwd(lib, q):
    _check(lib.alignq_site_bwd_apply_bn(q.g, q.S, q.z, q.ab, q.save, q.C, q.HW, q.nhwc, q.y_relu, q.y_bins, q.y_bin_bytes, q.dresidual,
                                        q.stats, q.B, q.F, q.act_range, q.eps, q.dx, q.dx_part, None), "site_bwd_apply_bn")


def _assert_bwd_guards(o, what):
    o["dx"].assert_written_and_bands_intact(what + " dx")
    if o["dres"] is not None:
        o["dres"].assert_written_and_bands_intact(what + " dres")


@pytest.mark.parametrize("use_res,want_bins", [(True, False), (False, True)])
def test_site_backward_outputs_guards_and_launch_forms(dev, lib, use_res, want_bins):
    """The one-tile backward at B = 128, F = 1024: the vectorised form (write-through dres and dx), the dword form (dx four bytes off a
    16-byte boundary: plain stores; the same per-element arithmetic) and the twin launch."""
    c, c2 = SiteCase(dev, 21), SiteCase(dev, 22)
    t, S = _site_bwd_setup(lib, dev, c, use_res, want_bins)
    q, o = _site_bwd_args(lib, dev, c, t, S, use_res, want_bins)
    _launch_bwd(lib, q)
    qd, od = _site_bwd_args(lib, dev, c, t, S, use_res, want_bins, shift=1)
    _launch_bwd(lib, qd)
    torch.cuda.synchronize()
    _assert_bwd_guards(o, "vec")
    _assert_bwd_guards(od, "dword")
    dx = o["dx"].out.cpu().numpy()
    assert np.isfinite(dx).all() and np.abs(dx).max() > 0
    assert np.array_equal(_bits(o["dx"].out), _bits(od["dx"].out)), "dword form: dx"
    if use_res:
        assert np.array_equal(_bits(o["dres"].out), _bits(od["dres"].out)), "dword form: dres"
    # twin against the two single launches
    t2, S2 = _site_bwd_setup(lib, dev, c2, False, False)
    q1, o1 = _site_bwd_args(lib, dev, c, t, S, use_res, want_bins)
    q2, o2 = _site_bwd_args(lib, dev, c2, t2, S2, False, False)
    _check(lib.alignq_site_bwd_apply_bn_twin(ctypes.byref(q1), ctypes.byref(q2), None), "bwd twin")
    r2, p2 = _site_bwd_args(lib, dev, c2, t2, S2, False, False)
    _launch_bwd(lib, r2)
    torch.cuda.synchronize()
    _assert_bwd_guards(o1, "twin a")
    _assert_bwd_guards(o2, "twin b")
    assert np.array_equal(_bits(o1["dx"].out), _bits(o["dx"].out)) and np.array_equal(_bits(o1["part"]), _bits(o["part"]))
    assert np.array_equal(_bits(o2["dx"].out), _bits(p2["dx"].out)) and np.array_equal(_bits(o2["part"]), _bits(p2["part"]))
    if use_res:
        assert np.array_equal(_bits(o1["dres"].out), _bits(o["dres"].out))


# ------------------------------------------------------------------------------------------------------------ the convolutions
def _filter(g, shape, dev, k=K):
    n = (1 << k) - 1
    return (torch.randint(-n, n + 1, shape, generator=g).float() / n).to(dev)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("C,W", [(16, 32), (32, 16), (64, 8)])
def test_body_convolution_outputs_guards_and_launch_forms(dev, lib, C, W, B):
    """alignq_conv3x3_nhwc forward and data gradient (with and without the joining tensor) and the one-launch backward at H = 8:
    outputs written whole, bands intact, and the one-launch backward's dx / dW equal the stand-alone entries' bit for bit."""
    H = 8
    g = torch.Generator().manual_seed(100 * C + B)
    n = B * H * W * C
    x, gy, add = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    w = _filter(g, (C, 3, 3, C), dev)
    y = Guarded(dev, n)
    part = torch.zeros(C * lib.alignq_conv3x3_bn_parts(B, H, W, C) * 2, device=dev)
    _check(lib.alignq_conv3x3_nhwc(_p(x), _p(w), _p(y.out), B, H, W, C, K, 0, None, _p(part), None, 0, 0, None), "fwd")
    dxs = {}
    for a in (None, add):
        d = Guarded(dev, n)
        _check(lib.alignq_conv3x3_nhwc(_p(gy), _p(w), _p(d.out), B, H, W, C, K, 1, _p(a), None, None, 0, 0, None), "dgrad")
        dxs[a is not None] = d
    nbytes = lib.alignq_conv3x3_wgrad_ws_bytes(C)
    dw_ref, ws_ref = torch.empty_like(w), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _check(lib.alignq_conv3x3_nhwc_wgrad(_p(x), _p(gy), _p(dw_ref), _p(ws_ref), B, H, W, C, None, None, 0, 0, None), "wgrad")
    one = {}
    for a in (None, add):
        d, ws, ns, dw = Guarded(dev, n), Guarded(dev, nbytes // 4), ctypes.c_int(0), torch.empty_like(w)
        _check(lib.alignq_conv3x3_nhwc_bwd(_p(x), _p(gy), _p(w), _p(d.out), _p(ws.out), B, H, W, C, K, ctypes.byref(ns), _p(a),
                                           *([None] * 7), None, 0, 0, None), "bwd")
        from alignq_amd import _lib as L
        _check(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws.out]), L.ptr_array([dw]), (ctypes.c_int * 1)(ns.value),
                                                     (ctypes.c_int * 1)(9 * C * C), None), "reduce")
        one[a is not None] = (d, ws, ns.value, dw)
    torch.cuda.synchronize()
    y.assert_written_and_bands_intact("forward y")
    assert np.isfinite(y.out.cpu().numpy()).all() and float(y.out.abs().max()) > 0
    for joined in (False, True):
        dxs[joined].assert_written_and_bands_intact("dgrad dx")
        d, ws, n_slabs, dw = one[joined]
        d.assert_written_and_bands_intact("one-launch dx")
        ws.assert_written_and_bands_intact("filter-gradient slabs", n_slabs * 9 * C * C)
        assert np.array_equal(_bits(d.out), _bits(dxs[joined].out)), "one-launch dx against the stand-alone data gradient"
        assert np.array_equal(_bits(dw), _bits(dw_ref)), "one-launch dW against the stand-alone filter gradient"


@pytest.mark.parametrize("CIN,COUT,W", [(16, 32, 32), (32, 64, 16)])
def test_transition_outputs_guards_and_launch_forms(dev, lib, CIN, COUT, W):
    """Transitions at output height 8, B = 2: the one-launch forward against the two stand-alone convolutions (bit for bit), the
    stand-alone data gradients and the one-launch backward write their outputs whole and nothing else."""
    B, H = 2, 16
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(7 * CIN)
    nx, ny = B * H * W * CIN, B * Ho * Wo * COUT
    x, add = torch.randn(nx, generator=g).to(dev), torch.randn(nx, generator=g).to(dev)
    gy3, gy1 = torch.randn(ny, generator=g).to(dev), torch.randn(ny, generator=g).to(dev)
    w3, w1 = _filter(g, (COUT, 3, 3, CIN), dev), _filter(g, (COUT, 1, 1, CIN), dev)
    y3, y1, y3r, y1r = (Guarded(dev, ny) for _ in range(4))
    _check(lib.alignq_transition_nhwc_fwd(_p(x), _p(w3), _p(w1), _p(y3.out), _p(y1.out), B, H, W, CIN, COUT, K, None, None, None), "fwd")
    _check(lib.alignq_conv_gen_nhwc_fwd(_p(x), _p(w3), _p(y3r.out), B, H, W, CIN, COUT, 3, 2, K, None, None), "fwd3")
    _check(lib.alignq_conv_gen_nhwc_fwd(_p(x), _p(w1), _p(y1r.out), B, H, W, CIN, COUT, 1, 2, K, None, None), "fwd1")
    dx1, dx3, dx = (Guarded(dev, nx) for _ in range(3))
    none7 = [None] * 7
    _check(lib.alignq_conv_gen_nhwc_dgrad(_p(gy1), _p(w1), _p(dx1.out), B, H, W, CIN, COUT, 1, 2, K, _p(add), *none7, None), "dg1")
    _check(lib.alignq_conv_gen_nhwc_dgrad(_p(gy3), _p(w3), _p(dx3.out), B, H, W, CIN, COUT, 3, 2, K, _p(dx1.out), *none7, None), "dg3")
    ws3 = Guarded(dev, lib.alignq_conv_gen_wgrad_ws_bytes(CIN, COUT, 3) // 4)
    ws1 = Guarded(dev, lib.alignq_conv_gen_wgrad_ws_bytes(CIN, COUT, 1) // 4)
    ns3, ns1 = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib.alignq_transition_nhwc_bwd(_p(x), _p(gy3), _p(gy1), _p(w3), _p(w1), _p(dx.out), _p(ws3.out), _p(ws1.out), B, H, W, CIN,
                                          COUT, K, ctypes.byref(ns3), ctypes.byref(ns1), _p(add), *([None] * 14), None), "bwd")
    torch.cuda.synchronize()
    for t, what in ((y3, "y3"), (y1, "y1"), (y3r, "y3 alone"), (y1r, "y1 alone"), (dx1, "dx 1x1"), (dx3, "dx 3x3"), (dx, "dx one launch")):
        t.assert_written_and_bands_intact(what)
    ws3.assert_written_and_bands_intact("3x3 slabs", ns3.value * 9 * CIN * COUT)
    ws1.assert_written_and_bands_intact("1x1 slabs", ns1.value * CIN * COUT)
    assert np.array_equal(_bits(y3.out), _bits(y3r.out)) and np.array_equal(_bits(y1.out), _bits(y1r.out))
    # (the one-launch data gradient sums the 1x1 term as a tenth tap: equal to fp32 accumulation order only)
    np.testing.assert_allclose(dx.out.cpu().numpy(), dx3.out.cpu().numpy(), rtol=1e-4, atol=1e-4)


def test_stem_forward_output_and_guards(dev, lib):
    B, H, W = 2, 8, 32
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(B * H * W * 3, generator=g).to(dev), _filter(g, (16, 3, 3, 3), dev)
    ys = [Guarded(dev, B * H * W * 16) for _ in range(2)]
    part = torch.zeros(16 * lib.alignq_conv_stem_bn_parts(B, H, W) * 2, device=dev)
    _check(lib.alignq_conv_stem_nhwc_fwd(_p(x), _p(w), _p(ys[0].out), B, H, W, K, None, None), "stem")
    _check(lib.alignq_conv_stem_nhwc_fwd(_p(x), _p(w), _p(ys[1].out), B, H, W, K, _p(part), None), "stem + statistics")
    torch.cuda.synchronize()
    for y in ys:
        y.assert_written_and_bands_intact("stem y")
    assert np.array_equal(_bits(ys[0].out), _bits(ys[1].out)) and float(ys[0].out.abs().max()) > 0
    # against the exact convolution: integer filter bins times fp32 inputs, fp32 accumulation (27 terms)
    ref = torch.nn.functional.conv2d(x.view(B, H, W, 3).permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), padding=1)
    np.testing.assert_allclose(ys[0].out.view(B, H, W, 16).permute(0, 3, 1, 2).cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=2e-5)


# ------------------------------------------------------------------------------------------------- captured producer -> consumer
def test_captured_pairs_replay_to_the_eager_bits(dev, lib):
    """conv forward -> site forward and site backward -> conv backward, each pair captured in one graph and replayed 20 times: the
    consumer reads what the producer stored write-through; every replay gives the bits of the eager run."""
    C, H, W, B = C_S, H_S, H_S * 0 + 32, B128                       # C = 16 body convolution: width 32
    g = torch.Generator().manual_seed(77)
    n = B * H * W * C
    F = C * H * W
    x, gy = torch.randn(n, generator=g).to(dev), (torch.randn(n, generator=g) * 1e-2).to(dev)
    w = _filter(g, (C, 3, 3, C), dev)
    gam, bet = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.2).to(dev)
    A, Gm = (torch.randn(128, 128, generator=g) * 0.05).to(dev), (torch.randn(128, 128, generator=g) * 0.05).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    n_parts = lib.alignq_conv3x3_bn_parts(B, H, W, C)
    z, y, dx, dxc = (torch.empty(n, **f32) for _ in range(4))
    part = torch.zeros(C * n_parts * 2, **f32)
    ab, save, stats = torch.empty(2, C, **f32), torch.empty(2, C, **f32), torch.empty(4, F, **f32)
    rm, rv, nbt = torch.zeros(C, **f32), torch.ones(C, **f32), torch.zeros((), dtype=torch.int64, device=dev)
    ws = torch.zeros(lib.alignq_site_ws_bytes(B, F), dtype=torch.uint8, device=dev)
    D, scal, S = torch.empty(B, B, **f32), torch.empty(4, **f32), torch.zeros(lib.alignq_site_bwd_ws_bytes(B) // 4, **f32)
    dA, dG, one = torch.empty_like(A), torch.empty_like(Gm), torch.ones((), **f32)
    bpart = torch.zeros(lib.alignq_site_bn_part_bytes(F, 1), dtype=torch.uint8, device=dev)
    wsw = torch.empty(lib.alignq_conv3x3_wgrad_ws_bytes(C), dtype=torch.uint8, device=dev)
    ns = ctypes.c_int(0)

    def forward(st):
        _check(lib.alignq_conv3x3_nhwc(_p(x), _p(w), _p(z), B, H, W, C, K, 0, None, _p(part), None, 0, 0, st), "conv fwd")
        _check(lib.alignq_site_partials_bn(_p(z), _p(part), _p(gam), _p(bet), _p(rm), _p(rv), _p(nbt), 0.1, 1e-5, _p(ab), _p(save), C,
                                           H * W, B, F, K, 2.0, 0.0, 1, None, 1, n_parts, _p(y), None, _p(stats), _p(ws), st), "site fwd")

    def backward(st):
        _check(lib.alignq_site_bwd_apply_bn(_p(gy), _p(S), _p(z), _p(ab), _p(save), C, H * W, 1, _p(y), None, 0, None, _p(stats), B, F,
                                            2.0, 0.0, _p(dx), _p(bpart), st), "site bwd")
        _check(lib.alignq_conv3x3_nhwc_bwd(_p(x), _p(dx), _p(w), _p(dxc), _p(wsw), B, H, W, C, K, ctypes.byref(ns), None,
                                           *([None] * 7), None, 0, 0, st), "conv bwd")

    forward(None)
    _check(lib.alignq_site_reduce_loss(_p(ws), B, F, _p(D), _p(A), _p(Gm), 128, 0.2, 0.3, _p(scal), None), "reduce")
    _check(lib.alignq_site_prep_fused(_p(D), _p(A), _p(Gm), 128, _p(scal), 0.2, _p(one), B, F, _p(S), _p(dA), _p(dG), None), "prep")
    backward(None)
    torch.cuda.synchronize()
    n_slab = (F // 64) * 8256 if F > 4096 else (F // 32) * 8256
    eager_f = [_bits(y), _bits(stats), _bits(ws.view(torch.float32)[:n_slab])]
    eager_b = [_bits(dx), _bits(dxc), _bits(wsw.view(torch.float32)[:ns.value * 9 * C * C])]
    assert np.isfinite(eager_b[1].view(np.float32)).all() and np.abs(eager_b[1].view(np.float32)).max() > 0
    side = torch.cuda.Stream()
    graphs = []
    for fn in (forward, backward):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                fn(side.cuda_stream)
        graphs.append(gr)
    for _ in range(20):
        for t in (y, dx, dxc):
            t.fill_(float("nan"))
        rm.zero_(); rv.fill_(1.0)
        graphs[0].replay()
        graphs[1].replay()
        torch.cuda.synchronize()
        got_f = [_bits(y), _bits(stats), _bits(ws.view(torch.float32)[:n_slab])]
        got_b = [_bits(dx), _bits(dxc), _bits(wsw.view(torch.float32)[:ns.value * 9 * C * C])]
        for a_, b_ in zip(eager_f + eager_b, got_f + got_b):
            assert np.array_equal(a_, b_)
