"""The 3x3 convolutions of csrc/k3conv_kernels.hip (alignq_k3conv_fwd / _dgrad / _wgrad) against int64 references, bit for bit, in
every launch form: the three output-width tiles, contractions that end inside a 32-deep chunk, output widths that end inside a tile,
images of one pixel, one row, one column, below, at and above one spatial tile each way, several images (a halo that reached into the
neighbouring image or row would change the values), more tiles than one pass of the grid holds, the write-through window, both
filter-gradient tiles, every kept term pair.

Operands are integers and every output's sum of |products| stays below 2^24 (tests/k3conv_exact_oracle.py; proved for every row by
tests/test_k3conv_oracle_cpu.py), so all partial sums are exact in fp32 in any order and the result must be fp32(sum) / fp32(n) with
one IEEE division (fp32(sum) for the filter gradient).  Every output is a NaN-filled window between two guards of another value: an
unwritten element and a write outside the window both fail.  Every launch runs twice and must give the same bits.  The launch form
each row claims is asserted through alignq_k3conv_form, the slab count through the workspace query and n_slabs_out.  There is no
tolerance in this file."""
import ctypes
import functools

import pytest
import torch

from tests import k3conv_exact_oracle as O

pytestmark = pytest.mark.gpu
GUARD, GUARD_VALUE = 64, 12345.0          # floats on either side of an output window (a multiple of 4: the window stays 16-byte aligned)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from alignq_amd import _lib as L
    return L.load()


def _ids(cases):
    return [c["id"] for c in cases]


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from alignq_amd import _lib as L
    L.check(rc, what)


def _window(n, dev):
    """(buffer, window): n NaN floats between two guards"""
    buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, device=dev, dtype=torch.float32)
    win = buf[GUARD:GUARD + n]
    win.fill_(float("nan"))
    assert win.data_ptr() % 16 == 0
    return buf, win


def _guards_intact(buf, n, what):
    assert bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[GUARD + n:] == GUARD_VALUE).all()), what + ": a guard was overwritten"


def _same(got, ref, what):
    got = got.detach().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return
    bad = torch.nonzero(~(got == ref))
    i = tuple(bad[0].tolist())
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r"
                         % (what, len(bad), ref.numel(), i, float(got[i]), float(ref[i])))


def _bins(b, dev):
    """the filter operand: the integer bins' bf16 bit patterns, [cout][3][3][cin]"""
    t = b.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(t.to(torch.int64), b)
    return t.view(torch.int16).contiguous().to(dev)


def _geom(c):
    return c["B"], c["h"], c["w"], c["cin"], c["cout"]


@functools.lru_cache(maxsize=4)
def _g_ref(cid):
    c = {r["id"]: r for r in O.G_CASES}[cid]
    a, b = O.g_operands(c)
    return a, b, O.quotient(O.g_reference(c, a, b), O.nlev_of(c))


@pytest.mark.parametrize("c", O.G_CASES, ids=_ids(O.G_CASES))
def test_forward_and_data_gradient_are_the_quotient_of_the_integer_sum(dev, lib, c):
    """y = fp32(sum x b) / fp32(n), dx = fp32(sum dy b) / fp32(n): dense class-1 operands, and class-3 (18-bit) activations against
    sparse bins so that all three terms of the split carry value.  The data gradient writes exactly B H W CIN elements."""
    a, b, ref = _g_ref(c["id"])
    fwd = c["op"] == "fwd"
    op = O.K3_FWD if fwd else O.K3_DGRAD
    assert lib.alignq_k3conv_supported(*_geom(c)) == 1 and lib.alignq_k3conv_form(op, *_geom(c)) == c["form"]
    n_out = O.rows_of(c) * (c["cout"] if fwd else c["cin"])
    assert ref.numel() == n_out
    ad, wb = a.to(torch.float32).to(dev), _bins(b, dev)
    call = lib.alignq_k3conv_fwd if fwd else lib.alignq_k3conv_dgrad
    outs = []
    for _ in range(2):
        buf, win = _window(n_out, dev)
        _ok(call(_p(ad), _p(wb), _p(win), *_geom(c), c["w_bit"], _st()), "alignq_k3conv_" + c["op"])
        torch.cuda.synchronize()
        _guards_intact(buf, n_out, c["id"])
        outs.append(win)
    _same(outs[0], ref, "y[b, h, w, co]" if fwd else "dx[b, h, w, ci]")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same inputs differ"


def _reduce(lib, ws, dw, n_slabs, n_elem):
    from alignq_amd import _lib as L
    _ok(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws]), L.ptr_array([dw]), (ctypes.c_int * 1)(n_slabs),
                                              (ctypes.c_int * 1)(n_elem), _st()), "alignq_conv3x3_wgrad_reduce_multi")


@pytest.mark.parametrize("c", O.ALL_WGRAD, ids=_ids(O.ALL_WGRAD))
def test_filter_gradient_is_the_integer_sum(dev, lib, c):
    """dW = fp32(sum dy x).  dense: class 1 x class 1 in both tiles, slabs of one to 512.  dyA_xB: (dy class, x class) (1, 3), (3, 1),
    (2, 2) with a sparse dy - the six kept pairs.  The one-call form twice and the deferred form (slabs, then
    alignq_conv3x3_wgrad_reduce_multi): all the same bits; the slab count is the table's."""
    x, dy = O.wgrad_operands(c)
    ref = O.wgrad_reference(c, x, dy).to(torch.float32).reshape(-1)
    n_elem = 9 * c["cin"] * c["cout"]
    n_slabs, _ = O.wgrad_slabs(c)
    assert lib.alignq_k3conv_form(O.K3_WGRAD, *_geom(c)) == c["form"]
    nws = lib.alignq_k3conv_wgrad_ws_bytes(*_geom(c))
    assert nws == n_slabs * 4 * n_elem, ("slabs", nws / (4.0 * n_elem), n_slabs)
    xd, dyd = x.to(torch.float32).to(dev), dy.to(torch.float32).to(dev)
    outs = []
    for deferred in (False, False, True):
        wbuf, ws = _window(nws // 4, dev)
        dbuf, dw = _window(n_elem, dev)
        ns = ctypes.c_int(0)
        _ok(lib.alignq_k3conv_wgrad(_p(xd), _p(dyd), None if deferred else _p(dw), _p(ws), *_geom(c),
                                    ctypes.byref(ns) if deferred else None, _st()), "alignq_k3conv_wgrad")
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


def _nchw(t, dev):
    """an NHWC integer tensor as the channels-last fp32 NCHW tensor the Functions take"""
    return t.to(torch.float32).to(dev).permute(0, 3, 1, 2)


def test_qconv_k3_function_reaches_the_same_bits(dev):
    """ops.QConvK3Fn (its own filter packing through alignq_qconv_pack_weights, workspace and reduction): y, dx and dW equal the
    integer references at 36 -> 12, 3 x 5 x 5"""
    from alignq_amd import ops
    by_id = {c["id"]: c for c in O.G_CASES}
    cf, cd = by_id["fwd_36x12_B3H5W5_dense"], by_id["dgrad_36x12_B3H5W5_dense"]
    x, b = O.g_operands(cf)
    gy = O.g_operands(cd)[0].clamp(-15, 15)
    O.assert_exact_budget(O.dgrad_i64, gy, b, stride=1, pad=1, h_in=cd["h"], w_in=cd["w"])
    O.assert_exact_budget(O.wgrad_i64, x, gy, ks=3, stride=1, pad=1)
    xt = _nchw(x, dev).requires_grad_(True)
    wt = (_nchw(b, dev) / 255.0).requires_grad_(True)
    assert ops.qconv_k3_supported(xt, wt, (1, 1), (1, 1), (1, 1), 1, None, 8)
    assert not ops.qconv_k3_supported(xt, wt, (2, 2), (1, 1), (1, 1), 1, None, 8)
    assert not ops.qconv_k3_supported(xt, wt, (1, 1), (0, 0), (1, 1), 1, None, 8)
    assert not ops.qconv_k3_supported(xt, wt, (1, 1), (1, 1), (1, 1), 1, None, 32)
    assert not ops.qconv_k3_supported(xt.contiguous(), wt, (1, 1), (1, 1), (1, 1), 1, None, 8)
    y = ops.QConvK3Fn.apply(xt, wt, 8)
    y.backward(_nchw(gy, dev))
    assert y.is_contiguous(memory_format=torch.channels_last) and xt.grad.shape == xt.shape and wt.grad.shape == wt.shape
    _same(y.permute(0, 2, 3, 1), O.quotient(O.conv_i64(x, b, 1, 1), 255.0), "y")
    _same(xt.grad.permute(0, 2, 3, 1), O.quotient(O.dgrad_i64(gy, b, 1, 1, cd["h"], cd["w"]), 255.0), "dx")
    _same(wt.grad.permute(0, 2, 3, 1), O.wgrad_i64(x, gy, 3, 1, 1).to(torch.float32), "dW")
