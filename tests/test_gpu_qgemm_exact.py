"""The convolutions of csrc/qgemm_kernels.hip (alignq_qconv_fwd / _dgrad / _wgrad / _stem7_fwd / _stem7_wgrad) against int64
references, bit for bit, in every launch form: the four tiles, the four k-forms, split-K 1 to 4, the filter gradient's TC / TN
blockings, gather forms and ring kernel, every operand mode (three bf16 terms, f16 level index from fp32 or int16) and every
kept term pair.

Operands are integers and every output's sum of |products| stays below 2^24 (tests/qgemm_exact_oracle.py; proved for every case
by tests/test_qgemm_exact_oracle_cpu.py), so all partial sums are exact in fp32 in any order and the result must be
fp32(sum) / fp32(den) with one IEEE division.  A dropped term, k step, tap, row block or split changes bits.  Outputs start as NaN:
an unwritten element fails.  The exports are called through alignq_amd._lib so that scratch, n_slabs_out and bn_part are the
test's; the launch form each row of the case table claims is asserted through the library's own queries.

The sixth pair of a level operand's filter gradient, x_lo * dy_l, sits at 2^-24 of a product - the order of the pairs the
three-term form drops by design - and cannot be pinned exactly inside the budget; it has no case.  The only tolerance in this
file is the derived bound of the x_levels = 255 filter gradients (see that test)."""
import ctypes
import functools

import pytest
import torch

from tests import qgemm_exact_oracle as O

pytestmark = pytest.mark.gpu


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


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), device=dev, dtype=dtype)


def _same(got, ref, what):
    got = got.detach().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return
    bad = torch.nonzero(~(got == ref))
    i = tuple(bad[0].tolist())
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r"
                         % (what, len(bad), ref.numel(), i, float(got[i]), float(ref[i])))


def _bins(b, mode, dev):
    """the filter operand: the integer bins' bf16 (fp32 activation) or f16 (level activation) bit patterns"""
    t = b.to(torch.float32).to(torch.bfloat16 if mode == "f32" else torch.float16)
    assert torch.equal(t.to(torch.int64), b)
    return t.view(torch.int16).contiguous().to(dev)


def _act(a, mode, xlev, dev):
    """(tensor, x_levels, x_bin_bytes): integers as fp32, the level tensor idx / xlev, or the int16 indices"""
    if mode == "f32":
        return a.to(torch.float32).to(dev), 0.0, 0
    if mode == "lev":
        return (a.to(torch.float32) / torch.tensor(xlev)).to(dev), xlev, 0
    return a.to(torch.int16).to(dev), xlev, 2


def _dims(c):
    return c["B"], c["h"], c["w"], c["cin"], c["cout"], c["ks"], c["stride"]


# ---------------------------------------------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=4)
def _g_ref(cid):
    c = {r["id"]: r for r in O.G_CASES + O.BN}[cid]
    a, b = O.g_operands(c)
    return a, b, O.g_reference(c, a, b)


def _forward(lib, dev, c, a, b, part=None):
    ho, wo = O.out_hw(c)
    x, xlev, xb = _act(a, c["mode"], O.XLEV_FWD, dev)
    n_parts = lib.alignq_qconv_bn_parts(*_dims(c), c["groups"], xlev)
    Mg = c["B"] // c["groups"] * ho * wo
    assert n_parts == -(-Mg // c["bm"]), ("row tiles per group", n_parts, Mg, c["bm"])      # (tells 64 from 128 where Mg > 64)
    y = _nan((c["B"], ho, wo, c["cout"]), dev)
    if part is not None:
        part = _nan((c["groups"], n_parts, c["cout"], 2), dev, torch.float64)
    wb = _bins(b, c["mode"], dev)
    _ok(lib.alignq_qconv_fwd(_p(x), _p(wb), _p(y), *_dims(c), c["w_bit"], xlev, xb, c["groups"], _p(part), _st()), "alignq_qconv_fwd")
    torch.cuda.synchronize()
    return y, part


@pytest.mark.parametrize("c", O.FWD, ids=_ids(O.FWD))
def test_forward_is_the_quotient_of_the_integer_sum(dev, lib, c):
    """y = fp32(sum x b) / fp32(255) (fp32 activation) or / fp32(255 * 255) (level activation), in the tile and k-form the row
    states; the row tiles are asserted through alignq_qconv_bn_parts"""
    a, b, total = _g_ref(c["id"])
    y, _ = _forward(lib, dev, c, a, b)
    _same(y, O.quotient(total, O.nlev_of(c), O.XLEV_FWD if c["mode"] != "f32" else 0.0), "y[n, oh, ow, co]")


@pytest.mark.parametrize("c", O.BN, ids=_ids(O.BN))
def test_forward_batch_norm_partials_are_each_tile_s_own_sums(dev, lib, c):
    """w_bit = 1, activations in [0, 3]: y is an integer and bn_part[group][tile][channel] = {sum y, sum y^2} over exactly the
    rows of that tile inside its group - a row counted beyond the group, or a tile straddling two groups, changes an integer"""
    a, b, total = _g_ref(c["id"])
    y, part = _forward(lib, dev, c, a, b, part=True)
    _same(y, total.to(torch.float32), "y[n, oh, ow, co]")
    _same(part, O.bn_expected(total.to(torch.int64), c["groups"], c["bm"]).to(torch.float64), "bn_part[group, tile, co, {s, q}]")


# ---------------------------------------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize("c", O.DGRAD, ids=_ids(O.DGRAD))
def test_data_gradient_is_the_quotient_of_the_integer_sum_with_and_without_scratch(dev, lib, c):
    """dx = fp32(sum dy b) / fp32(255): with the scratch (the split the row states, asserted through
    alignq_qconv_dgrad_ws_bytes; the closing pass adds the raw sums and divides once) and without it (one workgroup per tile) -
    both the same bits.  Every element of dx is written, the zeros of the stride-2 forms included."""
    a, b, total = _g_ref(c["id"])
    ref = O.quotient(total, O.nlev_of(c))
    dy, wb = a.to(torch.float32).to(dev), _bins(b, "f32", dev)
    n_dx = c["B"] * c["h"] * c["w"] * c["cin"]
    nws = lib.alignq_qconv_dgrad_ws_bytes(*_dims(c))
    assert nws == (c["split"] * 4 * n_dx if c["split"] > 1 else 0), ("split", nws / (4.0 * n_dx), c["split"])
    for ws in ([torch.empty(nws, dtype=torch.uint8, device=dev)] if nws else []) + [None]:
        dx = _nan((c["B"], c["h"], c["w"], c["cin"]), dev)
        _ok(lib.alignq_qconv_dgrad(_p(dy), _p(wb), _p(dx), *_dims(c), c["w_bit"], _p(ws), _st()), "alignq_qconv_dgrad")
        torch.cuda.synchronize()
        _same(dx, ref, "dx[n, h, w, ci] (%s scratch)" % ("with" if ws is not None else "without"))


# -------------------------------------------------------------------------------------------------------- filter gradient
def _reduce(lib, ws, dw, n_slabs, n_elem):
    from alignq_amd import _lib as L
    _ok(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([ws]), L.ptr_array([dw]), (ctypes.c_int * 1)(n_slabs),
                                              (ctypes.c_int * 1)(n_elem), _st()), "alignq_conv3x3_wgrad_reduce_multi")


def _wgrad_both_forms(lib, dev, c, x, dy):
    """dW by the one-call form and by the deferred form (slabs, then alignq_conv3x3_wgrad_reduce_multi); asserts the slab count
    through alignq_qconv_wgrad_ws_bytes and n_slabs_out and that the two forms agree bit for bit"""
    n_elem = c["cout"] * c["ks"] ** 2 * c["cin"]
    nws = lib.alignq_qconv_wgrad_ws_bytes(*_dims(c))
    assert nws == c["splits"] * 4 * n_elem, ("slabs", nws / (4.0 * n_elem), c["splits"])
    xd, xlev, xb = _act(x, c["mode"], O.wgrad_xlev(c), dev)
    dyd = dy.to(torch.float32).to(dev)
    outs = []
    for deferred in (False, True):
        ws, dw, ns = _nan((nws // 4,), dev), _nan((n_elem,), dev), ctypes.c_int(0)
        _ok(lib.alignq_qconv_wgrad(_p(xd), _p(dyd), None if deferred else _p(dw), _p(ws), *_dims(c), xlev, xb,
                                   ctypes.byref(ns) if deferred else None, _st()), "alignq_qconv_wgrad")
        if deferred:
            assert ns.value == c["splits"]
            _reduce(lib, ws, dw, ns.value, n_elem)
        torch.cuda.synchronize()
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]), "the deferred reduction differs from the stand-alone one"
    return outs[0], c["splits"]


WGRAD_EXACT = O.WGRAD_DENSE + O.WGRAD_PAIRS + O.WGRAD_LEVEL


@pytest.mark.parametrize("c", WGRAD_EXACT, ids=_ids(WGRAD_EXACT))
def test_filter_gradient_is_the_integer_sum(dev, lib, c):
    """dW = fp32(sum dy x) (over 256 for a level operand: exact).  dense: class 1 x class 1 in every TC / TN blocking, gather form
    and the ring kernel, for the three operand modes.  dyA_xB: (dy class, x class) (1, 3), (3, 1), (2, 2) with a sparse dy - the
    six kept pairs of the three-term form.  lev22 / lev3: both index terms against dy's high and middle terms, and dy's low term
    against the index's high term."""
    x, dy = O.wgrad_operands(c)
    dw, _ = _wgrad_both_forms(lib, dev, c, x, dy)
    _same(dw, O.wgrad_expected(c, x, dy).reshape(-1), "dW[co, ky, kx, ci]")


@pytest.mark.parametrize("c", O.WGRAD_255, ids=_ids(O.WGRAD_255))
def test_level_filter_gradient_at_255_levels_is_within_its_rounding_bound(dev, lib, c):
    """x = idx / 255, dy in [0, 15]: every slab's sum is a non-negative exact integer, divided by 255 once (one rounding), and the
    n_slabs slabs are added (n_slabs - 1 more); with nothing negative every rounding is at most 2^-24 of the final value, inside
    the bound the CIFAR index-operand test derived, |dW - I / 255| <= (n_slabs + 5) 2^-24 I / 255.
    Measured worst |error| / bound on the MI355X: 0.25 (tap kernel 1x1, 3 slabs), 0.26 (tap kernel gathered 3x3 stride 2, 2 slabs),
    0.31 (ring kernel, 3 slabs)."""
    x, dy = O.wgrad_operands(c)
    dw, n_slabs = _wgrad_both_forms(lib, dev, c, x, dy)
    ref = O.wgrad_reference(c, x, dy).reshape(-1).double() / 255.0
    got = dw.cpu().double()
    bound = (n_slabs + 5) * 2.0 ** -24 * ref
    print(c["id"], "n_slabs", n_slabs, "largest |error| / bound:", float(((got - ref).abs() / bound.clamp_min(1e-300)).max()))
    assert torch.isfinite(got).all() and float(((got - ref).abs() - bound).max()) <= 0.0


# ---------------------------------------------------------------------------------------------------------------- the stem
def _stem_fwd(lib, dev, c, x, b, with_part):
    B, h, w = c["B"], c["h"], c["w"]
    ho, wo = O.out_hw(c)
    n_parts = lib.alignq_qconv_stem7_bn_parts(B, h, w, c["groups"])
    tiles = (B // c["groups"] * ho * wo + 15) // 16
    assert n_parts == min((tiles + 3) // 4, 512)
    y = _nan((B, ho, wo, 64), dev)
    part = _nan((c["groups"], n_parts, 64, 2), dev, torch.float64) if with_part else None
    xd, wb = x.to(torch.float32).to(dev), _bins(b, "f32", dev)
    _ok(lib.alignq_qconv_stem7_fwd(_p(xd), _p(wb), _p(y), B, h, w, c["w_bit"], c["groups"], _p(part), _st()), "alignq_qconv_stem7_fwd")
    torch.cuda.synchronize()
    return y, part


@pytest.mark.parametrize("c", O.STEM_FWD, ids=_ids(O.STEM_FWD))
def test_stem_forward_is_the_quotient_of_the_integer_sum(dev, lib, c):
    """the 7x7 stride-2 stem: dense class-1 images, and class-3 images (all three bf16 terms) against sparse bins; 8 x 8 (every
    pixel a border pixel), odd 37 x 41, 64 x 48.  The kernel divides by a multiplication with one residual correction, which is
    the correctly rounded quotient for these operands."""
    x, b = O.stem_operands(c)
    y, _ = _stem_fwd(lib, dev, c, x, b, False)
    _same(y, O.quotient(O.stem7_fwd_i64(x, b), O.nlev_of(c)), "y[n, oh, ow, co]")


@pytest.mark.parametrize("c", O.STEM_BN, ids=_ids(O.STEM_BN))
def test_stem_batch_norm_partials_are_each_workgroup_s_own_sums(dev, lib, c):
    """w_bit = 1: integer y; bn_part[group][workgroup][channel] over the rows of the 16-pixel tiles that workgroup walks (one tile
    per wave on the small grids, two for the first 32 waves at 512 x 260)"""
    x, b = O.stem_operands(c)
    total = O.stem7_fwd_i64(x, b)
    y, part = _stem_fwd(lib, dev, c, x, b, True)
    _same(y, total.to(torch.float32), "y[n, oh, ow, co]")
    _same(part, O.stem_bn_expected(total, c["groups"]).to(torch.float64), "bn_part[group, workgroup, co, {s, q}]")


STEM_W = O.STEM_WGRAD + O.STEM_WGRAD_PAIRS


@pytest.mark.parametrize("c", STEM_W, ids=_ids(STEM_W))
def test_stem_filter_gradient_is_the_integer_sum(dev, lib, c):
    """dW [64][7][7][3] = fp32(sum dy x): dense class 1 x class 1 on every grid, the three term-pair sets on the larger ones; one
    slab per 32-pixel step - 512 slabs of 64 pixels, the last 190 empty, at 2 x 253 x 161 - (asserted through the workspace query and
    n_slabs_out), both reduction forms bit-equal"""
    x, dy = O.stem_operands(c)
    B, h, w = c["B"], c["h"], c["w"]
    n_elem = 64 * 147
    nws = lib.alignq_qconv_stem7_wgrad_ws_bytes(B, h, w)
    assert nws == c["splits"] * 4 * n_elem
    xd, dyd = x.to(torch.float32).to(dev), dy.to(torch.float32).to(dev)
    outs = []
    for deferred in (False, True):
        ws, dw, ns = _nan((nws // 4,), dev), _nan((n_elem,), dev), ctypes.c_int(0)
        _ok(lib.alignq_qconv_stem7_wgrad(_p(xd), _p(dyd), None if deferred else _p(dw), _p(ws), B, h, w,
                                         ctypes.byref(ns) if deferred else None, _st()), "alignq_qconv_stem7_wgrad")
        if deferred:
            assert ns.value == c["splits"]
            _reduce(lib, ws, dw, ns.value, n_elem)
        torch.cuda.synchronize()
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]), "the deferred reduction differs from the stand-alone one"
    _same(outs[0], O.stem7_wgrad_i64(x, dy).to(torch.float32), "dW[co * 147 + (ky * 7 + kx) * 3 + c]")


# ------------------------------------------------------------------------------------------------- through the Functions
def _nchw(t, dev):
    """an NHWC integer tensor as the channels-last fp32 NCHW tensor the Functions take"""
    return t.to(torch.float32).to(dev).permute(0, 3, 1, 2)


def test_qconv_gemm_function_reaches_the_same_bits(dev):
    """ops.QConvGemmFn (3x3 halo forward, data gradient, ring filter gradient; its own filter packing, workspaces and reductions):
    y, dx and dW equal the integer references"""
    from alignq_amd import ops
    c = next(r for r in O.FWD if r["km"] == 2 and r["B"] == 9 and r["mode"] == "f32" and r["set"] == "dense" and r["cin"] == 64)
    x, b = O.g_operands(c)
    gy = O.g_operands(next(r for r in O.DGRAD if r["km"] == 2 and r["B"] == 9))[0]
    geo = dict(stride=1, pad=1)
    O.assert_exact_budget(O.dgrad_i64, gy, b, h_in=4, w_in=4, **geo)
    O.assert_exact_budget(O.wgrad_i64, x, gy, ks=3, **geo)
    xt = _nchw(x, dev).requires_grad_(True)
    wt = (_nchw(b, dev) / 255.0).requires_grad_(True)
    assert xt.is_contiguous(memory_format=torch.channels_last) and wt.is_contiguous(memory_format=torch.channels_last)
    y = ops.QConvGemmFn.apply(xt, wt, 8, 1, 0.0)
    y.backward(_nchw(gy, dev))
    _same(y.permute(0, 2, 3, 1), O.quotient(O.conv_i64(x, b, 1, 1), 255.0), "y")
    _same(xt.grad.permute(0, 2, 3, 1), O.quotient(O.dgrad_i64(gy, b, 1, 1, 4, 4), 255.0), "dx")
    _same(wt.grad.permute(0, 2, 3, 1), O.wgrad_i64(x, gy, 3, 1, 1).to(torch.float32), "dW")


def test_qconv_stem7_function_reaches_the_same_bits(dev):
    from alignq_amd import ops
    c = next(r for r in O.STEM_WGRAD if (r["B"], r["h"]) == (2, 37))
    x, dy = O.stem_operands(c)
    b = O.stem_operands(next(r for r in O.STEM_FWD if (r["B"], r["h"], r["set"]) == (2, 37, "dense")))[1]
    O.assert_exact_budget(O.conv_i64, x, b, stride=2, pad=3)
    xt = _nchw(x, dev)
    wt = (_nchw(b, dev) / 255.0).requires_grad_(True)
    y = ops.QConvStem7Fn.apply(xt, wt, 8)
    y.backward(_nchw(dy, dev))
    _same(y.permute(0, 2, 3, 1), O.quotient(O.stem7_fwd_i64(x, b), 255.0), "y")
    _same(wt.grad.permute(0, 2, 3, 1).reshape(-1), O.stem7_wgrad_i64(x, dy).to(torch.float32), "dW")
