"""The body and transition convolutions after their schedule changed (filter loads unconditional on clamped addresses, one accumulator
per pixel group with the fragments of the next k step in flight, the C = 16 backward at three workgroups per CU): checks that do
not depend on the order of accumulation, so that a dropped, doubled or misplaced k step or pixel group changes bits.

Exact-integer checks: integer-valued operands chosen so that every sum of products stays below 2^24 (255 * 255 * 144 at C = 16 with
8-bit activations, 255 * 15 * 576 at C = 32 / 64 with 4-bit ones): every partial sum is then an exactly representable fp32 integer
in ANY order, and the result must equal an int64 convolution cast to fp32 and divided by the same fp32 denominator, bit for bit.
B = 3 gives several tiles per image and several images (the halo rows at image boundaries are hit).

One-launch backward: alignq_conv3x3_nhwc_bwd must reproduce the stand-alone entries bit for bit (same device code per role), with
and without the lazy batch-norm operands and the filler role, at B = 3 (one tile per pixel range) and, at C = 16, B = 40 (320
filter-gradient tiles over 256 ranges: two tiles per range, ranges of unequal length, trailing ranges empty)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32), (32, 16), (64, 8)]          # (C, H = W) of the ResNet body
B3 = 3


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


def _st():
    from alignq_amd import _lib as L
    return L.stream_ptr()


def _check(rc, what):
    from alignq_amd import _lib as L
    L.check(rc, what)


def _conv_i64(x, b, stride, pad):
    """x [B, H, W, Cin], b [Cout, KS, KS, Cin] (int64, CPU) -> [B, Ho, Wo, Cout]: sum over taps of integer matrix products"""
    B, H, W, Cin = x.shape
    Cout, KS = b.shape[0], b.shape[1]
    Ho, Wo = (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, Cin, dtype=torch.int64)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = torch.zeros(B, Ho, Wo, Cout, dtype=torch.int64)
    for ky in range(KS):
        for kx in range(KS):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += xs.reshape(-1, Cin) .matmul(b[:, ky, kx].t()).reshape(B, Ho, Wo, Cout)
    return out


def _dgrad_i64(dy, b):
    """dx[b,h,w,ci] = sum dy[b,h-ky+1,w-kx+1,co] * b[co,ky,kx,ci]: the convolution of dy with the flipped, transposed filter"""
    return _conv_i64(dy, b.flip(1, 2).permute(3, 1, 2, 0).contiguous(), 1, 1)


def _bins(cout, ks, cin, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-n, n + 1, (cout, ks, ks, cin), generator=g, dtype=torch.int64)


def _check_parts(part, y, rows_per_tile):
    """bn_part [C][tiles][2] = per-tile per-channel {sum y, sum y^2} in fp32 against the column sums of y [B, H, W, C] in double.
    A lane sums at most 4 outputs, a 16-lane row is a 4-level tree, at most 4 waves are added: at most 12 fp32 additions on any
    path (13 roundings for the squares), each within 2^-24 relative of a partial sum that is bounded by the sum of magnitudes."""
    Bn, H, W, C = y.shape
    t = y.double().reshape(Bn * H // rows_per_tile, rows_per_tile * W, C)
    u = 2.0 ** -24
    s, q = t.sum(1).t(), (t * t).sum(1).t()                       # [C][tiles]
    sa = t.abs().sum(1).t()
    assert tuple(part.shape) == (C, t.shape[0], 2)
    e0 = float(((part[:, :, 0].double() - s).abs() - 12 * u * sa).max())
    e1 = float(((part[:, :, 1].double() - q).abs() - 13 * u * q).max())
    print("bn_part excess over the bound (<= 0):", e0, e1)
    assert e0 <= 0.0 and e1 <= 0.0


# --------------------------------------------------------------------------------------------------------- forward, body
@pytest.mark.parametrize("C,H", SHAPES)
@pytest.mark.parametrize("form", ["fp32", "int16", "int8"])
def test_forward_of_integer_operands_is_exact(dev, lib, C, H, form):
    a_bit = 8 if C == 16 else 4
    n, xlev = 255, 2 ** a_bit - 1
    g = torch.Generator().manual_seed(100 + C + len(form))
    top = min(xlev, 127) if form == "int8" else xlev             # (an int8 index holds at most 127)
    idx = torch.randint(0, top + 1, (B3, H, H, C), generator=g, dtype=torch.int64)
    b = _bins(C, 3, C, n, C)
    assert n * top * 9 * C < 2 ** 24
    w = (b.float() / float(n)).to(dev)
    y = torch.full((B3, H, H, C), float("nan"), device=dev)
    n_parts = lib.alignq_conv3x3_bn_parts(B3, H, H, C)
    assert n_parts > 1
    part = torch.full((C, n_parts, 2), float("nan"), device=dev)
    if form == "fp32":
        x = idx.float().to(dev)
        _check(lib.alignq_conv3x3_nhwc(_p(x), _p(w), _p(y), B3, H, H, C, 8, 0, None, _p(part), None, 0, 0, _st()), "fwd")
        den = torch.tensor(float(n))
    else:
        xi = idx.to(torch.int16 if form == "int16" else torch.int8).to(dev)
        _check(lib.alignq_conv3x3_nhwc(None, _p(w), _p(y), B3, H, H, C, 8, 0, None, _p(part), _p(xi), xi.element_size(), a_bit,
                                       _st()), "fwd")
        den = torch.tensor(float(n)) * torch.tensor(float(xlev))
    torch.cuda.synchronize()
    ref = _conv_i64(idx, b, 1, 1).float() / den
    assert torch.equal(y.cpu(), ref)
    _check_parts(part.cpu(), y.cpu(), (B3 * H) // n_parts)


# -------------------------------------------------------------------------------------------------- data gradient, body
@pytest.mark.parametrize("C,H", SHAPES)
@pytest.mark.parametrize("with_add", [False, True])
def test_data_gradient_of_integer_operands_is_exact(dev, lib, C, H, with_add):
    n = 255
    g = torch.Generator().manual_seed(200 + C)
    dy = torch.randint(-15, 16, (B3, H, H, C), generator=g, dtype=torch.int64)
    b = _bins(C, 3, C, n, C + 1)
    assert n * 15 * 9 * C < 2 ** 24
    w = (b.float() / float(n)).to(dev)
    add = torch.randn(B3, H, H, C, generator=g) if with_add else None
    dx = torch.full((B3, H, H, C), float("nan"), device=dev)
    addd = add.to(dev) if with_add else None
    _check(lib.alignq_conv3x3_nhwc(_p(dy.float().to(dev)), _p(w), _p(dx), B3, H, H, C, 8, 1, _p(addd), None, None, 0, 0, _st()),
           "dgrad")
    torch.cuda.synchronize()
    ref = _dgrad_i64(dy, b).float() / torch.tensor(float(n))
    if with_add:
        ref = ref + add
    assert torch.equal(dx.cpu(), ref)


# ---------------------------------------------------------------------------------------------------- transition forward
@pytest.mark.parametrize("CIN,COUT,W", [(16, 32, 32), (32, 64, 16)])
def test_transition_forward_of_integer_operands_is_exact(dev, lib, CIN, COUT, W):
    n = 255
    g = torch.Generator().manual_seed(300 + CIN)
    xi = torch.randint(0, 16, (B3, W, W, CIN), generator=g, dtype=torch.int64)
    b3, b1 = _bins(COUT, 3, CIN, n, CIN + 2), _bins(COUT, 1, CIN, n, CIN + 3)
    assert n * 15 * 9 * CIN < 2 ** 24
    x = xi.float().to(dev)
    w3, w1 = (b3.float() / float(n)).to(dev), (b1.float() / float(n)).to(dev)
    Ho = W // 2
    ref3 = _conv_i64(xi, b3, 2, 1).float() / torch.tensor(float(n))
    ref1 = _conv_i64(xi, b1, 2, 0).float() / torch.tensor(float(n))
    np3 = lib.alignq_conv_gen_bn_parts(B3, W, W, CIN, COUT, 3, 2)
    np1 = lib.alignq_conv_gen_bn_parts(B3, W, W, CIN, COUT, 1, 2)
    assert np3 > 1 and np1 > 1

    def outs():
        return (torch.full((B3, Ho, Ho, COUT), float("nan"), device=dev), torch.full((B3, Ho, Ho, COUT), float("nan"), device=dev),
                torch.full((COUT, np3, 2), float("nan"), device=dev), torch.full((COUT, np1, 2), float("nan"), device=dev))
    y3, y1, p3, p1 = outs()
    _check(lib.alignq_conv_gen_nhwc_fwd(_p(x), _p(w3), _p(y3), B3, W, W, CIN, COUT, 3, 2, 8, _p(p3), _st()), "fwd 3x3")
    _check(lib.alignq_conv_gen_nhwc_fwd(_p(x), _p(w1), _p(y1), B3, W, W, CIN, COUT, 1, 2, 8, _p(p1), _st()), "fwd 1x1")
    z3, z1, q3, q1 = outs()
    _check(lib.alignq_transition_nhwc_fwd(_p(x), _p(w3), _p(w1), _p(z3), _p(z1), B3, W, W, CIN, COUT, 8, _p(q3), _p(q1), _st()),
           "transition fwd")
    torch.cuda.synchronize()
    for y, ref, part, parts in ((y3, ref3, p3, np3), (y1, ref1, p1, np1), (z3, ref3, q3, np3), (z1, ref1, q1, np1)):
        assert torch.equal(y.cpu(), ref)
        _check_parts(part.cpu(), y.cpu(), (B3 * Ho) // parts)
    assert torch.equal(p3, q3) and torch.equal(p1, q1)


# ------------------------------------------------------------------------------ one-launch backward vs stand-alone entries
def _tile_f(F):
    return 64 if F >= 16384 else 32          # site backward's features per tile (site_internal.h: bwd_tile_features)


@pytest.mark.parametrize("C,H,B", [(16, 32, 3), (32, 16, 3), (64, 8, 3), (16, 32, 40)])
@pytest.mark.parametrize("lazy", ["plain", "lazy_totals", "lazy_parts_fill"])
def test_one_launch_backward_equals_the_stand_alone_entries(dev, lib, C, H, B, lazy):
    from alignq_amd import _lib as L
    n = 255
    g = torch.Generator().manual_seed(400 + C + B)
    f32 = dict(dtype=torch.float32, device=dev)
    x = torch.randn(B, H, H, C, generator=g).to(dev)
    gy = (torch.randn(B, H, H, C, generator=g) * 0.01).to(dev)
    w = (_bins(C, 3, C, n, C + 4).float() / float(n)).to(dev)
    add = torch.randn(B, H, H, C, generator=g).to(dev)
    z = ab = save = ktot = part = dgam = dbet = None
    dz = gy
    if lazy != "plain":
        z = torch.randn(B, H, H, C, generator=g).to(dev)
        ab = (torch.rand(2, C, generator=g) + 0.5).to(dev)
        save = (torch.rand(2, C, generator=g) + 0.5).to(dev)
        if lazy == "lazy_totals":
            ktot = (torch.randn(2, C, generator=g) * 0.01).to(dev)
            k = ktot
        else:
            # per-tile sums [tiles][min(C, tile_f)][2], tile t = features t * tile_f .. of a [pixel][C] row; multiples of 2^-12 below
            # 2^4, at most 2^10 of them per channel: their double sum is exact, so the totals do not depend on its order.
            # 1 / (B H W) is rounded to double once, as the launcher does.
            F = C * H * H
            tf = _tile_f(F)
            cp = min(C, tf)
            nt = F // tf
            pi = torch.randint(-2 ** 15, 2 ** 15, (nt, cp, 2), generator=g, dtype=torch.int64)
            part = (pi.double() / 4096.0).float().to(dev)
            tot = torch.zeros(C, 2, dtype=torch.float64)
            for t in range(nt):
                c0 = (t * tf) % C
                tot[c0:c0 + cp] += pi[t].double() / 4096.0
            inv_n = 1.0 / (float(B) * H * H)
            k = (tot * inv_n).float().t().contiguous().to(dev)                       # [2][C]: k0, k1
            dgam, dbet = torch.full((C,), float("nan"), **f32), torch.full((C,), float("nan"), **f32)
        # dz exactly as the kernels form it (one IEEE operation per step, no fused multiply-add)
        dz = ab[0] * ((gy - k[0]) - (((z - save[0]) * save[1]) * k[1]))
    st = _st()
    # stand-alone entries on the explicit dz
    dx_ref, dw_ref = torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
    ws0 = torch.empty(lib.alignq_conv3x3_wgrad_ws_bytes(C), dtype=torch.uint8, device=dev)
    _check(lib.alignq_conv3x3_nhwc(_p(dz), _p(w), _p(dx_ref), B, H, H, C, 8, 1, _p(add), None, None, 0, 0, st), "dgrad")
    _check(lib.alignq_conv3x3_nhwc_wgrad(_p(x), _p(dz), _p(dw_ref), _p(ws0), B, H, H, C, None, None, 0, 0, st), "wgrad")
    # one launch
    dx, dw = torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
    ws = torch.empty(lib.alignq_conv3x3_wgrad_ws_bytes(C), dtype=torch.uint8, device=dev)
    ns = ctypes.c_int(0)
    fill_dw = fill_ref = None
    if lazy == "lazy_parts_fill":
        # filler role: the slab reduction of an earlier convolution (here: the stand-alone launch's slabs, deferred) rides along
        ws1 = torch.empty_like(ws0)
        ns1 = ctypes.c_int(0)
        _check(lib.alignq_conv3x3_nhwc_wgrad(_p(x), _p(dz), None, _p(ws1), B, H, H, C, ctypes.byref(ns1), None, 0, 0, st), "wgrad slabs")
        fill_dw = torch.full_like(w, float("nan"))
        _check(lib.alignq_conv3x3_nhwc_bwd_fill(
            _p(x), _p(gy), _p(w), _p(dx), _p(ws), B, H, H, C, 8, ctypes.byref(ns), _p(add), _p(z), _p(ab), _p(save), None, _p(part),
            _p(dgam), _p(dbet), None, 0, 0, 1, L.ptr_array([ws1]), L.ptr_array([fill_dw]), (ctypes.c_int * 1)(ns1.value),
            (ctypes.c_int * 1)(9 * C * C), st), "bwd_fill")
        fill_ref = dw_ref
    else:
        _check(lib.alignq_conv3x3_nhwc_bwd(_p(x), _p(gy), _p(w), _p(dx), _p(ws), B, H, H, C, 8, ctypes.byref(ns), _p(add), _p(z),
                                           _p(ab), _p(save), _p(ktot), None, None, None, None, 0, 0, st), "bwd")
    _check(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws]), L.ptr_array([dw]), (ctypes.c_int * 1)(ns.value),
                                                 (ctypes.c_int * 1)(9 * C * C), st), "reduce")
    torch.cuda.synchronize()
    assert torch.isfinite(dx_ref).all() and torch.isfinite(dw_ref).all()
    assert torch.equal(dx, dx_ref)
    assert torch.equal(dw, dw_ref)
    if fill_dw is not None:
        assert torch.equal(fill_dw, fill_ref)
        tot_f = tot.float()
        assert torch.equal(dbet.cpu(), tot_f[:, 0]) and torch.equal(dgam.cpu(), tot_f[:, 1])
