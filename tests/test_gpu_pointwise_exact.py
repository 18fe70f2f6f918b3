"""The pointwise convolutions of csrc/pointwise_kernels.hip (alignq_pwconv_fwd / _dgrad / _wgrad) against int64 references, bit for
bit, in every launch form: the three output-width tiles, contractions that end inside a 32-deep half step, output widths that end
inside a tile, row counts of 1, below, at and above one tile and beyond one pass of the grid cap, the four filter-gradient tiles,
every kept term pair.

Operands are integers and every output's sum of |products| stays below 2^24 (tests/pointwise_exact_oracle.py; proved for every row
by tests/test_pointwise_oracle_cpu.py), so all partial sums are exact in fp32 in any order and the result must be
fp32(sum) / fp32(n) with one IEEE division (fp32(sum) for the filter gradient).  Every output is a NaN-filled window between two
guards of another value: an unwritten element and a write outside the window both fail.  Every launch runs twice and must give the
same bits.  The launch form each row claims is asserted through alignq_pwconv_form, the slab count through the workspace query and
n_slabs_out.  There is no tolerance in this file."""
import ctypes
import functools

import pytest
import torch

from tests import pointwise_exact_oracle as O

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
    """the filter operand: the integer bins' bf16 bit patterns, [cout][cin]"""
    t = b.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(t.to(torch.int64), b)
    return t.view(torch.int16).contiguous().to(dev)


@functools.lru_cache(maxsize=4)
def _g_ref(cid):
    c = {r["id"]: r for r in O.G_CASES}[cid]
    a, b = O.g_operands(c)
    return a, b, O.quotient(O.g_reference(c, a, b), O.nlev_of(c))


@pytest.mark.parametrize("c", O.G_CASES, ids=_ids(O.G_CASES))
def test_forward_and_data_gradient_are_the_quotient_of_the_integer_sum(dev, lib, c):
    """y = fp32(sum x b) / fp32(255), dx = fp32(sum dy b) / fp32(255): dense class-1 operands, and class-3 (18-bit) activations against
    sparse bins so that all three terms of the split carry value.  The data gradient writes exactly M * CIN elements."""
    a, b, ref = _g_ref(c["id"])
    fwd = c["op"] == "fwd"
    M, cin, cout = O.rows_of(c), c["cin"], c["cout"]
    op = O.PW_FWD if fwd else O.PW_DGRAD
    assert lib.alignq_pwconv_supported(M, cin, cout) == 1 and lib.alignq_pwconv_form(op, M, cin, cout) == c["form"]
    n_out = M * (cout if fwd else cin)
    assert ref.numel() == n_out
    ad, wb = a.to(torch.float32).to(dev), _bins(b, dev)
    call = lib.alignq_pwconv_fwd if fwd else lib.alignq_pwconv_dgrad
    outs = []
    for _ in range(2):
        buf, win = _window(n_out, dev)
        _ok(call(_p(ad), _p(wb), _p(win), M, cin, cout, c["w_bit"], _st()), "alignq_pwconv_" + c["op"])
        torch.cuda.synchronize()
        _guards_intact(buf, n_out, c["id"])
        outs.append(win)
    _same(outs[0], ref, "y[m, co]" if fwd else "dx[m, ci]")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same inputs differ"


def _reduce(lib, ws, dw, n_slabs, n_elem):
    from alignq_amd import _lib as L
    _ok(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws]), L.ptr_array([dw]), (ctypes.c_int * 1)(n_slabs),
                                              (ctypes.c_int * 1)(n_elem), _st()), "alignq_conv3x3_wgrad_reduce_multi")


@pytest.mark.parametrize("c", O.ALL_WGRAD, ids=_ids(O.ALL_WGRAD))
def test_filter_gradient_is_the_integer_sum(dev, lib, c):
    """dW = fp32(sum dy x).  dense: class 1 x class 1 in the four tiles, slabs of one to 512 (the last ones empty).  dyA_xB: (dy class,
    x class) (1, 3), (3, 1), (2, 2) with a sparse dy - the six kept pairs.  The one-call form twice and the deferred form (slabs, then
    alignq_conv3x3_wgrad_reduce_multi): all the same bits; the slab count is the table's."""
    x, dy = O.wgrad_operands(c)
    ref = O.wgrad_reference(c, x, dy).to(torch.float32).reshape(-1)
    M, cin, cout = O.rows_of(c), c["cin"], c["cout"]
    n_elem = cin * cout
    n_slabs, _ = O.wgrad_slabs(c)
    assert lib.alignq_pwconv_form(O.PW_WGRAD, M, cin, cout) == c["form"]
    nws = lib.alignq_pwconv_wgrad_ws_bytes(M, cin, cout)
    assert nws == n_slabs * 4 * n_elem, ("slabs", nws / (4.0 * n_elem), n_slabs)
    xd, dyd = x.to(torch.float32).to(dev), dy.to(torch.float32).to(dev)
    outs = []
    for deferred in (False, False, True):
        wbuf, ws = _window(nws // 4, dev)
        dbuf, dw = _window(n_elem, dev)
        ns = ctypes.c_int(0)
        _ok(lib.alignq_pwconv_wgrad(_p(xd), _p(dyd), None if deferred else _p(dw), _p(ws), M, cin, cout,
                                    ctypes.byref(ns) if deferred else None, _st()), "alignq_pwconv_wgrad")
        if deferred:
            assert ns.value == n_slabs
            _reduce(lib, ws, dw, ns.value, n_elem)
        torch.cuda.synchronize()
        _guards_intact(wbuf, nws // 4, c["id"] + " slabs")
        _guards_intact(dbuf, n_elem, c["id"] + " dW")
        assert bool(torch.isfinite(ws).all()), "a slab element was not written"
        outs.append(dw)
    _same(outs[0], ref, "dW[co, ci]")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same inputs differ"
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32)), "the deferred reduction differs from the stand-alone one"


def _nchw(t, dev):
    """an NHWC integer tensor as the channels-last fp32 NCHW tensor the Functions take"""
    return t.to(torch.float32).to(dev).permute(0, 3, 1, 2)


def test_qconv_pw_function_reaches_the_same_bits(dev):
    """ops.QConvPwFn (its own filter packing through alignq_qconv_pack_weights, workspace and reduction): y, dx and dW equal the
    integer references at 96 -> 24, 75 pixels"""
    from alignq_amd import ops
    by_id = {c["id"]: c for c in O.G_CASES + O.ALL_WGRAD}
    cf, cd, cw = by_id["fwd_96x24_M75_dense"], by_id["dgrad_96x24_M75_dense"], by_id["wgrad_96x24_M75_dense"]
    x, b = O.g_operands(cf)
    gy = O.g_operands(cd)[0].clamp(-15, 15)
    O.assert_exact_budget(O.dgrad_i64, gy, b, stride=1, pad=0, h_in=cd["h"], w_in=cd["w"])
    O.assert_exact_budget(O.wgrad_i64, x, gy, ks=1, stride=1, pad=0)
    xt = _nchw(x, dev).requires_grad_(True)
    wt = (_nchw(b, dev) / 255.0).requires_grad_(True)
    assert ops.qconv_pw_supported(xt, wt, (1, 1), (0, 0), (1, 1), 1, None, 8)
    assert not ops.qconv_pw_supported(xt, wt, (2, 2), (0, 0), (1, 1), 1, None, 8)
    assert not ops.qconv_pw_supported(xt, wt, (1, 1), (0, 0), (1, 1), 1, None, 32)
    y = ops.QConvPwFn.apply(xt, wt, 8)
    y.backward(_nchw(gy, dev))
    assert y.is_contiguous(memory_format=torch.channels_last) and xt.grad.shape == xt.shape and wt.grad.shape == wt.shape
    _same(y.permute(0, 2, 3, 1), O.quotient(O.conv_i64(x, b, 1, 0), 255.0), "y")
    _same(xt.grad.permute(0, 2, 3, 1), O.quotient(O.dgrad_i64(gy, b, 1, 0, cd["h"], cd["w"]), 255.0), "dx")
    _same(wt.grad.permute(0, 2, 3, 1), O.wgrad_i64(x, gy, 1, 1, 0).to(torch.float32), "dW")
    assert cw["form"] == 1
