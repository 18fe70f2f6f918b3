"""The 5x5 / padding 0 convolutions of csrc/k5conv_kernels.hip and csrc/k5_fwd_body.h (alignq_k5conv_fwd / _dgrad / _wgrad) against
int64 references, bit for bit, in every launch form of both forms (body and image): the three output-width tiles, contractions that
end inside a 32-deep chunk, output widths that end inside a tile, outputs of one pixel, one row, one column, below, at and above one
spatial tile each way, several images (a footprint that reached into the neighbouring image or row would change the values), more
tiles than one pass of the grid holds, the write-through window, the three filter-gradient tiles, slabs of one to 512 with an uneven
last one, every kept term pair, every w_bit, with and without a bias.

Operands are integers and every output's sum of |products| stays below 2^24 (tests/k5conv_exact_oracle.py; proved for every row by
tests/test_k5conv_oracle_cpu.py), so all partial sums are exact in fp32 in any order and the result must be fp32(sum) / fp32(n) with
one IEEE division, then one fp32 add of the bias (fp32(sum) for the filter gradient).  Every output, and the slab workspace, is a
NaN-filled window between two guards of another value: an unwritten element and a write outside the window both fail.  Every launch
runs twice and must give the same bits.  The launch form each row claims is asserted through alignq_k5conv_form, the slab count
through the workspace query and n_slabs_out.  There is no tolerance in this file."""
import ctypes
import functools

import pytest
import torch

from tests import k5conv_exact_oracle as O
from tests.test_gpu_k3conv_exact import _bins, _guards_intact, _ids, _nchw, _ok, _p, _reduce, _same, _st, _window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from alignq_amd import _lib as L
    return L.load()


def _geom(c):
    return c["B"], c["H"], c["W"], c["cin"], c["cout"]


@functools.lru_cache(maxsize=4)
def _g_ref(cid):
    c = {r["id"]: r for r in O.G_CASES}[cid]
    a, b = O.g_operands(c)
    return a, b, O.quotient(O.g_reference(c, a, b), O.nlev_of(c))


def _twice(call, n_out, dev, cid):
    """the launch into two fresh windows: guards intact, every element written (the caller compares with a finite reference)"""
    outs = []
    for _ in range(2):
        buf, win = _window(n_out, dev)
        call(win)
        torch.cuda.synchronize()
        _guards_intact(buf, n_out, cid)
        outs.append(win)
    return outs


@pytest.mark.parametrize("c", O.FWD, ids=_ids(O.FWD))
def test_forward_is_the_quotient_of_the_integer_sum_plus_the_bias(dev, lib, c):
    """y = fp32(sum x b) / fp32(n) without a bias, (that quotient) + bias[co] in fp32 with one: dense class-1 operands, and class-3
    (18-bit) activations against sparse bins so that all three terms of the split carry value; body and image form"""
    a, b, ref = _g_ref(c["id"])
    assert lib.alignq_k5conv_supported(O.K5_FWD, *_geom(c)) == 1 and lib.alignq_k5conv_form(O.K5_FWD, *_geom(c)) == c["form"]
    n_out = O.rows_of(c) * c["cout"]
    assert ref.numel() == n_out and tuple(a.shape) == (c["B"], c["H"], c["W"], c["cin"])
    ad, wb = a.to(torch.float32).to(dev), _bins(b, dev)
    bias = O.bias_of(c["cout"])
    for bt, want in ((None, ref), (bias.to(dev), O.with_bias(ref, bias))):
        outs = _twice(lambda win: _ok(lib.alignq_k5conv_fwd(_p(ad), _p(wb), _p(bt), _p(win), *_geom(c), c["w_bit"], _st()),
                                      "alignq_k5conv_fwd"), n_out, dev, c["id"])
        _same(outs[0], want, "y[b, h, w, co]" + (" without a bias" if bt is None else " with a bias"))
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same inputs differ"


@pytest.mark.parametrize("c", O.DGRAD, ids=_ids(O.DGRAD))
def test_data_gradient_is_the_quotient_of_the_integer_sum(dev, lib, c):
    """dx = fp32(sum dy b) / fp32(n) over the flipped, transposed bins; exactly B H W CIN elements are written"""
    a, b, ref = _g_ref(c["id"])
    assert lib.alignq_k5conv_supported(O.K5_DGRAD, *_geom(c)) == 1 and lib.alignq_k5conv_form(O.K5_DGRAD, *_geom(c)) == c["form"]
    n_out = c["B"] * c["H"] * c["W"] * c["cin"]
    assert ref.numel() == n_out == O.rows_of(c) * c["cin"] and tuple(a.shape) == (c["B"], c["H"] - 4, c["W"] - 4, c["cout"])
    ad, wb = a.to(torch.float32).to(dev), _bins(b, dev)
    outs = _twice(lambda win: _ok(lib.alignq_k5conv_dgrad(_p(ad), _p(wb), _p(win), *_geom(c), c["w_bit"], _st()),
                                  "alignq_k5conv_dgrad"), n_out, dev, c["id"])
    _same(outs[0], ref, "dx[b, h, w, ci]")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same inputs differ"


def test_image_form_has_no_data_gradient(lib):
    from alignq_amd import _lib as L
    assert lib.alignq_k5conv_supported(O.K5_DGRAD, 3, 9, 9, 3, 32) == 0 and lib.alignq_k5conv_form(O.K5_DGRAD, 3, 9, 9, 3, 32) == -1
    assert lib.alignq_k5conv_dgrad(0x10000, 0x10000, 0x10000, 3, 9, 9, 3, 32, 8, None) == L.EUNSUPPORTED      # before any launch


@pytest.mark.parametrize("c", O.ALL_WGRAD, ids=_ids(O.ALL_WGRAD))
def test_filter_gradient_is_the_integer_sum(dev, lib, c):
    """dW = fp32(sum dy x).  dense: class 1 x class 1 in all three tiles, slabs of one to 512.  dyA_xB: (dy class, x class) (1, 3),
    (3, 1), (2, 2) with a sparse dy - the six kept pairs.  The one-call form twice and the deferred form (slabs, then
    alignq_conv3x3_wgrad_reduce_multi): all the same bits; the slab count is the table's.  The image form stores 75 of its 80 columns."""
    x, dy = O.wgrad_operands(c)
    ref = O.wgrad_reference(c, x, dy).to(torch.float32).reshape(-1)
    n_elem = 25 * c["cin"] * c["cout"]
    n_slabs, _ = O.wgrad_slabs(c)
    assert lib.alignq_k5conv_supported(O.K5_WGRAD, *_geom(c)) == 1 and lib.alignq_k5conv_form(O.K5_WGRAD, *_geom(c)) == c["form"]
    nws = lib.alignq_k5conv_wgrad_ws_bytes(*_geom(c))
    assert nws == n_slabs * 4 * n_elem, ("slabs", nws / (4.0 * n_elem), n_slabs)
    xd, dyd = x.to(torch.float32).to(dev), dy.to(torch.float32).to(dev)
    outs = []
    for deferred in (False, False, True):
        wbuf, ws = _window(nws // 4, dev)
        dbuf, dw = _window(n_elem, dev)
        ns = ctypes.c_int(0)
        _ok(lib.alignq_k5conv_wgrad(_p(xd), _p(dyd), None if deferred else _p(dw), _p(ws), *_geom(c),
                                    ctypes.byref(ns) if deferred else None, _st()), "alignq_k5conv_wgrad")
        if deferred:
            assert ns.value == n_slabs
            _reduce(lib, ws, dw, ns.value, n_elem)
        torch.cuda.synchronize()
        _guards_intact(wbuf, nws // 4, c["id"] + " slabs")
        _guards_intact(dbuf, n_elem, c["id"] + " dW")
        assert bool(torch.isfinite(ws).all()), "a slab element was not written"
        outs.append(dw)
    _same(outs[0], ref, "dW[co, ky, kx, ci]")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same inputs differ"
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32)), "the deferred reduction differs from the stand-alone one"


@pytest.mark.parametrize("shape", [(36, 48), (3, 48)], ids=["body", "image"])
def test_qconv_k5_function_reaches_the_same_bits(dev, shape):
    """ops.QConvK5Fn (its own filter packing through alignq_qconv_pack_weights, workspace, reduction and bias): y, dx (body form) and dW
    equal the integer references on the 3 x 9 x 9 output grid; the bias gradient is the int64 sum of dy"""
    from alignq_amd import ops
    cin, cout = shape
    body = cin != 3
    cf = O._row("fwd", shape, O.GPAIR)
    x, b = O.g_operands(cf)
    gy = torch.randint(-15, 16, (cf["B"], cf["h"], cf["w"], cout), generator=O._gen(800), dtype=O.I64)
    O.assert_exact_budget(O.conv_i64, x, b, stride=1, pad=0)
    O.assert_exact_budget(O.dgrad_i64, gy, b, stride=1, pad=0, h_in=cf["H"], w_in=cf["W"])
    O.assert_exact_budget(O.wgrad_i64, x, gy, ks=5, stride=1, pad=0)
    bias = O.bias_of(cout)
    xt = _nchw(x, dev).requires_grad_(body)
    wt = (_nchw(b, dev) / 255.0).requires_grad_(True)
    bt = bias.to(dev).requires_grad_(True)
    assert ops.qconv_k5_supported(xt, wt, (1, 1), (0, 0), (1, 1), 1, bt, 8)
    assert not ops.qconv_k5_supported(xt, wt, (1, 1), (1, 1), (1, 1), 1, bt, 8)
    assert not ops.qconv_k5_supported(xt, wt, (2, 2), (0, 0), (1, 1), 1, bt, 8)
    assert not ops.qconv_k5_supported(xt, wt, (1, 1), (0, 0), (1, 1), 1, bt, 32)
    y = ops.QConvK5Fn.apply(xt, wt, bt, 8)
    y.backward(_nchw(gy, dev))
    assert y.is_contiguous(memory_format=torch.channels_last) and wt.grad.shape == wt.shape
    _same(y.permute(0, 2, 3, 1), O.with_bias(O.quotient(O.conv_i64(x, b, 1, 0), 255.0), bias), "y")
    _same(wt.grad.permute(0, 2, 3, 1), O.wgrad_i64(x, gy, 5, 1, 0).to(torch.float32), "dW")
    _same(bt.grad, gy.sum((0, 1, 2)).to(torch.float32), "dbias")
    if body:
        assert xt.grad.shape == xt.shape
        _same(xt.grad.permute(0, 2, 3, 1), O.quotient(O.dgrad_i64(gy, b, 1, 0, cf["H"], cf["W"]), 255.0), "dx")
    else:
        assert xt.grad is None
