"""The CIFAR convolution kernels' gradients (csrc/conv_kernels.hip: wgrad_body, stem_wgrad_kernel, dgrad_s2_body) and every
split-bf16 term of the forward and data-gradient kernels, against int64 references, bit for bit.

Every operand holds integers and every output's sum of |products| stays below 2^24 (tests/conv_exact_oracle.py;
tests/test_conv_exact_oracle_cpu.py proves it, and the term classes, for every case here): all partial sums are exact fp32
integers in any order, so a dropped, doubled or misplaced k step, lane group, tap or bf16 term pair changes bits.  Output buffers
start as NaN: an unwritten element fails.  Epilogues are restated one IEEE operation at a time (int64 -> fp32, / fp32(255), + add).

The filter gradient keeps six of the nine (dy term, x term) pairs: hh, hm, mh, hl, lh, mm.  The term-pair tests use the operand
classes whose products those six hold exactly: class 1 x class 3, class 3 x class 1, class 2 x class 2.  Class 2 x class 3 is NOT
exact, by design: ml, lm and ll are dropped, at most about 2^-26 of a product each - that is not a defect to fix in the kernel.

The only tolerances here are the derived bound of the index-operand filter gradient (see that test) and the existing
_check_parts bound on the batch-norm partials; nothing is fitted to what the kernels return."""
import ctypes
import functools

import pytest
import torch

from tests import conv_exact_oracle as O
from tests.test_gpu_conv_sched import _check, _check_parts, _p, _st, _tile_f

pytestmark = pytest.mark.gpu

N = 255                                          # filter levels at w_bit = 8


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


def _f(t, dev):
    return t.to(torch.float32).to(dev)


def _wt(b, dev):
    return (b.to(torch.float32) / float(N)).to(dev)


def _nan(shape, dev):
    return torch.full(tuple(shape), float("nan"), device=dev)


def _quot(i64):
    """the kernels' epilogue: the integer sum as fp32, divided by fp32(255)"""
    return i64.to(torch.float32) / torch.tensor(float(N))


def _same(got, ref, what):
    got = got.detach().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return
    bad = torch.nonzero(~(got == ref))
    i = tuple(bad[0].tolist())
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r"
                         % (what, len(bad), ref.numel(), i, float(got[i]), float(ref[i])))


def _ptrs(ts):
    from alignq_amd import _lib as L
    return L.ptr_array(ts)


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _reduce(lib, ws, dw, n_slabs, n_elem):
    _check(lib.alignq_conv3x3_wgrad_reduce_multi(len(ws), _ptrs(ws), _ptrs(dw), _ints(*n_slabs), _ints(*n_elem), _st()), "reduce")


def _ws(lib, c, dev):
    if c["kind"] == "body":
        n = lib.alignq_conv3x3_wgrad_ws_bytes(c["cin"])
    elif c["kind"] == "gen":
        n = lib.alignq_conv_gen_wgrad_ws_bytes(c["cin"], c["cout"], c["ks"])
    else:
        n = 256 * 432 * 4
    return torch.empty(n, dtype=torch.uint8, device=dev)


NO_LAZY = dict(z=None, ab=None, save=None, ktot=None, part=None, dgamma=None, dbeta=None)


def _wgrad(lib, dev, c, x, dy, deferred, lazy=NO_LAZY):
    """dW [cout, ks, ks, cin] of case c by its stand-alone entry: both launches at once, or (deferred) the slabs first and
    alignq_conv3x3_wgrad_reduce_multi behind them.  Returns (dW, slab count or None)."""
    B, h, w, ci, co, ks = c["B"], c["h"], c["w"], c["cin"], c["cout"], c["ks"]
    dw, ws = _nan((co, ks, ks, ci), dev), _ws(lib, c, dev)
    ns = ctypes.c_int(0)
    nsp = ctypes.byref(ns) if deferred else None
    dwp = None if deferred else _p(dw)
    lz = lazy
    if c["kind"] == "body":
        assert lz["z"] is None
        _check(lib.alignq_conv3x3_nhwc_wgrad(_p(x), _p(dy), dwp, _p(ws), B, h, w, ci, nsp, None, 0, 0, _st()), "wgrad")
    elif c["kind"] == "gen":
        _check(lib.alignq_conv_gen_nhwc_wgrad(_p(x), _p(dy), dwp, _p(ws), B, h, w, ci, co, ks, 2, nsp, _p(lz["z"]), _p(lz["ab"]),
                                              _p(lz["save"]), _p(lz["ktot"]), _p(lz["part"]), _st()), "gen wgrad")
    else:
        _check(lib.alignq_conv_stem_nhwc_wgrad(_p(x), _p(dy), dwp, _p(ws), B, h, w, nsp, _p(lz["z"]), _p(lz["ab"]), _p(lz["save"]),
                                               _p(lz["ktot"]), _p(lz["part"]), _p(lz["dgamma"]), _p(lz["dbeta"]), _st()),
               "stem wgrad")
    if deferred:
        assert ns.value >= 1
        _reduce(lib, [ws], [dw], [ns.value], [co * ks * ks * ci])
    torch.cuda.synchronize()
    return dw, (ns.value if deferred else None)


# ------------------------------------------------------------------------------ (a) filter gradient, dense class 1 x class 1
DENSE = O.DENSE_BODY + O.DENSE_GEN + O.DENSE_STEM
_BY_ID = {c["id"]: c for c in DENSE + O.PAIR_CASES + O.ACT3_CASES + O.DENSE_TRANSITION}


@functools.lru_cache(maxsize=None)
def _dense_ref(cid):
    c = _BY_ID[cid]
    x, dy = O.dense_operands(c)
    return x, dy, O.wgrad_i64(x, dy, c["ks"], c["stride"], c["pad"]).to(torch.float32)


@pytest.mark.parametrize("form", ["two_launches", "deferred"])
@pytest.mark.parametrize("c", DENSE, ids=_ids(DENSE))
def test_dense_filter_gradient_is_the_integer_sum(dev, lib, c, form):
    """x in [0, 255], dy in [-15, 15]: dW is the int64 sum as fp32 (the filter gradient divides by no level count), through
    alignq_conv3x3_nhwc_wgrad, alignq_conv_gen_nhwc_wgrad (KS = 3 and 1) and alignq_conv_stem_nhwc_wgrad, in both forms"""
    x, dy, ref = _dense_ref(c["id"])
    dw, _ = _wgrad(lib, dev, c, _f(x, dev), _f(dy, dev), form == "deferred")
    _same(dw, ref, "dW[co, ky, kx, ci]")


@pytest.mark.parametrize("c", O.DENSE_BODY, ids=_ids(O.DENSE_BODY))
def test_one_launch_backward_roles_are_exact(dev, lib, c):
    """alignq_conv3x3_nhwc_bwd: its filter-gradient role against the integer sum and, on the same dy, its data-gradient role"""
    x, dy, ref = _dense_ref(c["id"])
    B, h, w, C = c["B"], c["h"], c["w"], c["cin"]
    b = O.gen_class1((C, 3, 3, C), -N, N, 9)
    dx, dw, ws = _nan(x.shape, dev), _nan(ref.shape, dev), _ws(lib, c, dev)
    ns = ctypes.c_int(0)
    xd, dyd, wt = _f(x, dev), _f(dy, dev), _wt(b, dev)
    _check(lib.alignq_conv3x3_nhwc_bwd(_p(xd), _p(dyd), _p(wt), _p(dx), _p(ws), B, h, w, C, 8,
                                       ctypes.byref(ns), None, None, None, None, None, None, None, None, None, 0, 0, _st()), "bwd")
    _reduce(lib, [ws], [dw], [ns.value], [9 * C * C])
    torch.cuda.synchronize()
    _same(dw, ref, "dW[co, ky, kx, ci]")
    _same(dx, _quot(O.dgrad_i64(dy, b, 1, 1, h, w)), "dx[n, h, w, ci]")


# ------------------------------------------------------- (a, d) the transition block's one-launch backward: all three roles
@functools.lru_cache(maxsize=None)
def _transition_ref(cid):
    c = _BY_ID[cid]
    x, dy3, dy1, b3, b1 = O.transition_operands(c)
    h, w = c["h"], c["w"]
    return dict(x=x, dy3=dy3, dy1=dy1, b3=b3, b1=b1, dw3=O.wgrad_i64(x, dy3, 3, 2, 1).to(torch.float32),
                dw1=O.wgrad_i64(x, dy1, 1, 2, 0).to(torch.float32), dx3=O.dgrad_i64(dy3, b3, 2, 1, h, w),
                dx1=O.dgrad_i64(dy1, b1, 2, 0, h, w), add=torch.randn(x.shape, generator=torch.Generator().manual_seed(31)))


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("c", O.DENSE_TRANSITION, ids=_ids(O.DENSE_TRANSITION))
def test_transition_backward_roles_are_exact(dev, lib, c, with_add):
    """alignq_transition_nhwc_bwd: both filter-gradient roles against the integer sums; the data-gradient role takes the 1x1
    filter as a tenth tap of ONE accumulator, so dx is one quotient of the SUMMED integer (+ add) - which is why it differs from
    the two separate launches' sum of two quotients in the last bit"""
    r = _transition_ref(c["id"])
    B, h, w, ci, co = c["B"], c["h"], c["w"], c["cin"], c["cout"]
    dx, dw3, dw1 = _nan(r["x"].shape, dev), _nan(r["dw3"].shape, dev), _nan(r["dw1"].shape, dev)
    ws3 = torch.empty(lib.alignq_conv_gen_wgrad_ws_bytes(ci, co, 3), dtype=torch.uint8, device=dev)
    ws1 = torch.empty(lib.alignq_conv_gen_wgrad_ws_bytes(ci, co, 1), dtype=torch.uint8, device=dev)
    ns3, ns1 = ctypes.c_int(0), ctypes.c_int(0)
    add = r["add"].to(dev) if with_add else None
    xd, d3, d1, w3, w1 = _f(r["x"], dev), _f(r["dy3"], dev), _f(r["dy1"], dev), _wt(r["b3"], dev), _wt(r["b1"], dev)
    _check(lib.alignq_transition_nhwc_bwd(_p(xd), _p(d3), _p(d1), _p(w3), _p(w1), _p(dx), _p(ws3), _p(ws1), B, h, w, ci, co, 8,
                                          ctypes.byref(ns3), ctypes.byref(ns1), _p(add), *([None] * 14), _st()), "transition bwd")
    _reduce(lib, [ws3, ws1], [dw3, dw1], [ns3.value, ns1.value], [9 * ci * co, ci * co])
    torch.cuda.synchronize()
    _same(dw3, r["dw3"], "3x3 dW[co, ky, kx, ci]")
    _same(dw1, r["dw1"], "1x1 dW[co, 0, 0, ci]")
    ref = _quot(r["dx3"] + r["dx1"])
    _same(dx, ref + r["add"] if with_add else ref, "dx[n, h, w, ci]")


# ------------------------------------------------------------------------------------------- (d) stride-2 data gradient
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("ks", [3, 1])
@pytest.mark.parametrize("c", O.DENSE_TRANSITION, ids=_ids(O.DENSE_TRANSITION))
def test_stride2_data_gradient_is_exact(dev, lib, c, ks, with_add):
    """alignq_conv_gen_nhwc_dgrad: dy in [-15, 15], bins in [-255, 255]; dx = fp32(int64 sum) / fp32(255) (+ add)"""
    r = _transition_ref(c["id"])
    B, h, w, ci, co = c["B"], c["h"], c["w"], c["cin"], c["cout"]
    dy, b, i64 = (r["dy3"], r["b3"], r["dx3"]) if ks == 3 else (r["dy1"], r["b1"], r["dx1"])
    dx = _nan(r["x"].shape, dev)
    add = r["add"].to(dev) if with_add else None
    dyd, wt = _f(dy, dev), _wt(b, dev)
    _check(lib.alignq_conv_gen_nhwc_dgrad(_p(dyd), _p(wt), _p(dx), B, h, w, ci, co, ks, 2, 8, _p(add),
                                          *([None] * 7), _st()), "gen dgrad")
    torch.cuda.synchronize()
    ref = _quot(i64)
    _same(dx, ref + r["add"] if with_add else ref, "dx[n, h, w, ci]")


# ------------------------------------------------------------------------- (b) filter gradient, one test per kept term pair
@pytest.mark.parametrize("c", O.PAIR_CASES, ids=_ids(O.PAIR_CASES))
def test_filter_gradient_term_pairs_are_exact(dev, lib, c):
    """(dy class, x class) = (1, 3) exercises hh, hm, hl; (3, 1) hh, mh, lh; (2, 2) hh, hm, mh, mm - with a sparse dy (at most
    15 non-zero pixels per output channel: the image's corners, both sides of a tile boundary, several pixel ranges, all four
    8-pixel lane groups of a k step) so that 18-bit operands stay inside the 2^24 budget.  Bit-equal to the int64 sum.
    Class 2 x class 3 is deliberately absent: ml, lm and ll are dropped by design (about 2^-26 of a product at most)."""
    x, dy = O.pair_operands(c)
    ref = O.wgrad_i64(x, dy, c["ks"], c["stride"], c["pad"]).to(torch.float32)
    dw, _ = _wgrad(lib, dev, c, _f(x, dev), _f(dy, dev), False)
    _same(dw, ref, "dW[co, ky, kx, ci]")


# ---------------------------------------------------------------------------------- (c) index-operand filter gradient
@pytest.mark.parametrize("entry", ["wgrad", "bwd"])
@pytest.mark.parametrize("C,W,nbytes,a_bit", O.BINS_CASES)
def test_index_operand_filter_gradient_is_within_its_rounding_bound(dev, lib, C, W, nbytes, a_bit, entry):
    """x given as int16 / int8 level indices (x_bins), dy in [0, 15]: every partial sum is a non-negative exact integer.  The
    kernel multiplies each wave's (C = 16) or workgroup's sum by fl(1 / xlev) (two roundings against the true quotient), adds four
    wave partials at C = 16 (three more) and then n_slabs slabs (n_slabs - 1 more); with nothing negative every rounding is at
    most 2^-24 of the final value:  |dW - I / xlev| <= (n_slabs + 5) 2^-24 I / xlev.  A dropped 8-pixel lane group is orders of
    magnitude above that.  a_bit = 1 (xlev = 1) must be bit-exact."""
    idx, dy = O.bins_operands(C, W, nbytes, a_bit)
    I = O.wgrad_i64(idx, dy, 3, 1, 1)
    B = idx.shape[0]
    xb = idx.to(torch.int16 if nbytes == 2 else torch.int8).to(dev)
    dyd = _f(dy, dev)
    dw = _nan((C, 3, 3, C), dev)
    ws = torch.empty(lib.alignq_conv3x3_wgrad_ws_bytes(C), dtype=torch.uint8, device=dev)
    ns = ctypes.c_int(0)
    if entry == "wgrad":
        _check(lib.alignq_conv3x3_nhwc_wgrad(None, _p(dyd), None, _p(ws), B, W, W, C, ctypes.byref(ns), _p(xb), nbytes, a_bit,
                                             _st()), "wgrad bins")
    else:
        wt, dx = _wt(O.gen_class1((C, 3, 3, C), -N, N, 9), dev), _nan(dy.shape, dev)
        _check(lib.alignq_conv3x3_nhwc_bwd(None, _p(dyd), _p(wt), _p(dx), _p(ws), B, W, W, C, 8, ctypes.byref(ns), None, None, None,
                                           None, None, None, None, None, _p(xb), nbytes, a_bit, _st()), "bwd bins")
    _reduce(lib, [ws], [dw], [ns.value], [9 * C * C])
    torch.cuda.synchronize()
    got = dw.cpu()
    if a_bit == 1:
        _same(got, I.to(torch.float32), "dW[co, ky, kx, ci]")
        return
    xlev = float((1 << a_bit) - 1)
    ref = I.double() / xlev
    excess = (got.double() - ref).abs() - (ns.value + 5) * 2.0 ** -24 * ref
    print("n_slabs", ns.value, "largest |error| / bound:", float(((got.double() - ref).abs() / ((ns.value + 5) * 2.0 ** -24 * ref)
                                                                   .clamp_min(1e-300)).max()))
    assert torch.isfinite(got).all() and float(excess.max()) <= 0.0


# ------------------------------------------------------------ (e) forward and data gradient with class-3 activations
@pytest.mark.parametrize("c", O.ACT3_CASES, ids=_ids(O.ACT3_CASES))
def test_forward_and_data_gradient_of_three_term_activations_are_exact(dev, lib, c):
    """18-bit activations (a non-zero middle AND low bf16 term) against sparse small filter bins: fp32(int64 sum) / fp32(255),
    bit for bit, through alignq_conv3x3_nhwc (forward and data gradient), alignq_conv_stem_nhwc_fwd, alignq_conv_gen_nhwc_fwd
    and alignq_conv_gen_nhwc_dgrad (KS = 3 and 1); the forwards' batch-norm partials within the _check_parts bound"""
    a, b = O.act3_operands(c)
    B, h, w, ci, co, ks = c["B"], c["h"], c["w"], c["cin"], c["cout"], c["ks"]
    ad, wt = _f(a, dev), _wt(b, dev)
    fwd = c["op"] == "fwd"
    if fwd:
        ref = _quot(O.conv_i64(a, b, c["stride"], c["pad"]))
    else:
        ref = _quot(O.dgrad_i64(a, b, c["stride"], c["pad"], h, w))
    out = _nan(ref.shape, dev)
    part = n_parts = None
    if fwd:
        n_parts = (lib.alignq_conv3x3_bn_parts(B, h, w, ci) if c["kind"] == "body" else
                   lib.alignq_conv_stem_bn_parts(B, h, w) if c["kind"] == "stem" else
                   lib.alignq_conv_gen_bn_parts(B, h, w, ci, co, ks, 2))
        assert n_parts > 1
        part = _nan((co, n_parts, 2), dev)
    if c["kind"] == "body":
        _check(lib.alignq_conv3x3_nhwc(_p(ad), _p(wt), _p(out), B, h, w, ci, 8, 0 if fwd else 1, None, _p(part), None, 0, 0, _st()),
               "conv3x3")
    elif c["kind"] == "stem":
        _check(lib.alignq_conv_stem_nhwc_fwd(_p(ad), _p(wt), _p(out), B, h, w, 8, _p(part), _st()), "stem fwd")
    elif fwd:
        _check(lib.alignq_conv_gen_nhwc_fwd(_p(ad), _p(wt), _p(out), B, h, w, ci, co, ks, 2, 8, _p(part), _st()), "gen fwd")
    else:
        _check(lib.alignq_conv_gen_nhwc_dgrad(_p(ad), _p(wt), _p(out), B, h, w, ci, co, ks, 2, 8, None, *([None] * 7), _st()),
               "gen dgrad")
    torch.cuda.synchronize()
    _same(out, ref, "y[n, h, w, co]" if fwd else "dx[n, h, w, ci]")
    if fwd:
        _check_parts(part.cpu(), out.cpu(), (B * ref.shape[1]) // n_parts)


# --------------------------------------------------------- (f) lazy batch-norm operands without an export-level test so far
def _lazy_record(dev, g, B, C, HW, form):
    """ab, save [2][C] and the totals k = {k0, k1} [2][C] either given (bn_ktot) or left to the kernel to form from per-tile sums
    (bn_dx_part) built as in test_one_launch_backward_equals_the_stand_alone_entries: multiples of 2^-12 below 2^4 in the site
    backward's tile layout [tiles][min(C, tile_f)][2], so that their double sum is exact in any order; 1 / (B HW) is rounded to
    double once, as the launcher does."""
    r = dict(NO_LAZY, ab=(torch.rand(2, C, generator=g) + 0.5).to(dev), save=(torch.rand(2, C, generator=g) + 0.5).to(dev), tot=None)
    if form == "totals":
        r["ktot"] = r["k"] = (torch.randn(2, C, generator=g) * 0.01).to(dev)
        return r
    F = C * HW
    tf = _tile_f(F)
    cp, nt = min(C, tf), F // tf
    pi = torch.randint(-2 ** 15, 2 ** 15, (nt, cp, 2), generator=g, dtype=torch.int64)
    r["part"] = (pi.double() / 4096.0).float().to(dev)
    tot = torch.zeros(C, 2, dtype=torch.float64)
    for t in range(nt):
        c0 = (t * tf) % C
        tot[c0:c0 + cp] += pi[t].double() / 4096.0
    r["k"] = (tot * (1.0 / (float(B) * HW))).float().t().contiguous().to(dev)
    r["tot"] = tot.float()
    return r


def _explicit_dz(r, gy, z):
    """dz exactly as the kernels form it on load: one IEEE operation per step, no fused multiply-add"""
    k, ab, save = r["k"], r["ab"], r["save"]
    return ab[0] * ((gy - k[0]) - (((z - save[0]) * save[1]) * k[1]))


def _param_grads(r, dev, C):
    if r["part"] is not None:
        r["dgamma"], r["dbeta"] = _nan((C,), dev), _nan((C,), dev)


def _check_param_grads(r):
    if r["part"] is not None:
        assert torch.equal(r["dbeta"].cpu(), r["tot"][:, 0]) and torch.equal(r["dgamma"].cpu(), r["tot"][:, 1])


LAZY_GEN = [O.gen(ci, co, w, ks) for ci, co, w in O.TRANSITION_SHAPES for ks in (3, 1)]


def _float_operands(c, seed):
    g = torch.Generator().manual_seed(seed)
    sh = (c["B"], c["ho"], c["wo"], c["cout"])
    x = torch.randn(c["B"], c["h"], c["w"], c["cin"], generator=g)
    return g, x, torch.randn(sh, generator=g) * 0.01, torch.randn(sh, generator=g)


@pytest.mark.parametrize("form", ["totals", "parts"])
@pytest.mark.parametrize("c", O.DENSE_STEM + LAZY_GEN, ids=_ids(O.DENSE_STEM + LAZY_GEN))
def test_lazy_filter_gradient_equals_the_entry_on_explicit_dz(dev, lib, c, form):
    """alignq_conv_stem_nhwc_wgrad and alignq_conv_gen_nhwc_wgrad with the lazy batch-norm operands (bn_ktot and bn_dx_part
    forms) against the same entry on dz formed by torch one operation at a time: bit-equal; the stem also writes the batch-norm
    parameter gradients in the parts form (the transition filter gradients leave them to the data-gradient kernel)"""
    g, x, gy, z = _float_operands(c, 600 + c["cin"] + c["ks"] + c["h"])
    x, gy, z = x.to(dev), gy.to(dev), z.to(dev)
    r = _lazy_record(dev, g, c["B"], c["cout"], c["ho"] * c["wo"], form)
    r["z"] = z
    if c["kind"] == "stem":
        _param_grads(r, dev, c["cout"])
    ref, _ = _wgrad(lib, dev, c, x, _explicit_dz(r, gy, z), False)
    got, _ = _wgrad(lib, dev, c, x, gy, False, r)
    assert torch.isfinite(ref).all()
    _same(got, ref.cpu(), "dW[co, ky, kx, ci]")
    if c["kind"] == "stem":
        _check_param_grads(r)


@pytest.mark.parametrize("form", ["totals", "parts"])
@pytest.mark.parametrize("c", LAZY_GEN, ids=_ids(LAZY_GEN))
def test_lazy_stride2_data_gradient_equals_the_entry_on_explicit_dz(dev, lib, c, form):
    g, x, gy, z = _float_operands(c, 700 + c["cin"] + c["ks"])
    B, h, w, ci, co, ks = c["B"], c["h"], c["w"], c["cin"], c["cout"], c["ks"]
    wt = _wt(O.gen_class1((co, ks, ks, ci), -N, N, 11), dev)
    add, gy, z = torch.randn_like(x).to(dev), gy.to(dev), z.to(dev)
    r = _lazy_record(dev, g, B, co, c["ho"] * c["wo"], form)
    _param_grads(r, dev, co)
    ref, got = _nan(x.shape, dev), _nan(x.shape, dev)
    dz = _explicit_dz(r, gy, z)
    _check(lib.alignq_conv_gen_nhwc_dgrad(_p(dz), _p(wt), _p(ref), B, h, w, ci, co, ks, 2, 8, _p(add),
                                          *([None] * 7), _st()), "gen dgrad")
    _check(lib.alignq_conv_gen_nhwc_dgrad(_p(gy), _p(wt), _p(got), B, h, w, ci, co, ks, 2, 8, _p(add), _p(z), _p(r["ab"]),
                                          _p(r["save"]), _p(r["ktot"]), _p(r["part"]), _p(r["dgamma"]), _p(r["dbeta"]), _st()),
           "gen dgrad lazy")
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    _same(got, ref.cpu(), "dx[n, h, w, ci]")
    _check_param_grads(r)


@pytest.mark.parametrize("form", ["totals", "parts"])
@pytest.mark.parametrize("CIN,COUT,W", O.TRANSITION_SHAPES)
def test_lazy_transition_backward_equals_the_entry_on_explicit_dz(dev, lib, CIN, COUT, W, form):
    """alignq_transition_nhwc_bwd with BOTH lazy records (the 3x3's and the 1x1's) against the same launch on explicit dz3 / dz1:
    dx and both filter gradients bit-equal; in the parts form both records' dgamma / dbeta equal the exact totals"""
    B, Ho = 3, W // 2
    g = torch.Generator().manual_seed(800 + CIN)
    sh = (B, Ho, Ho, COUT)
    x = torch.randn(B, W, W, CIN, generator=g).to(dev)
    add = torch.randn(B, W, W, CIN, generator=g).to(dev)
    gy3, z3 = (torch.randn(sh, generator=g) * 0.01).to(dev), torch.randn(sh, generator=g).to(dev)
    gy1, z1 = (torch.randn(sh, generator=g) * 0.01).to(dev), torch.randn(sh, generator=g).to(dev)
    w3 = _wt(O.gen_class1((COUT, 3, 3, CIN), -N, N, 12), dev)
    w1 = _wt(O.gen_class1((COUT, 1, 1, CIN), -N, N, 13), dev)
    r3, r1 = _lazy_record(dev, g, B, COUT, Ho * Ho, form), _lazy_record(dev, g, B, COUT, Ho * Ho, form)
    _param_grads(r3, dev, COUT)
    _param_grads(r1, dev, COUT)

    def run(d3, d1, lazy3, lazy1):
        dx, dw3, dw1 = _nan(x.shape, dev), _nan(w3.shape, dev), _nan(w1.shape, dev)
        ws3 = torch.empty(lib.alignq_conv_gen_wgrad_ws_bytes(CIN, COUT, 3), dtype=torch.uint8, device=dev)
        ws1 = torch.empty(lib.alignq_conv_gen_wgrad_ws_bytes(CIN, COUT, 1), dtype=torch.uint8, device=dev)
        ns3, ns1 = ctypes.c_int(0), ctypes.c_int(0)
        rec = [_p(l[k]) for l in (lazy3, lazy1) for k in ("z", "ab", "save", "ktot", "part", "dgamma", "dbeta")]
        _check(lib.alignq_transition_nhwc_bwd(_p(x), _p(d3), _p(d1), _p(w3), _p(w1), _p(dx), _p(ws3), _p(ws1), B, W, W, CIN, COUT, 8,
                                              ctypes.byref(ns3), ctypes.byref(ns1), _p(add), *rec, _st()), "transition bwd")
        _reduce(lib, [ws3, ws1], [dw3, dw1], [ns3.value, ns1.value], [9 * CIN * COUT, CIN * COUT])
        torch.cuda.synchronize()
        return dx, dw3, dw1

    ref = run(_explicit_dz(r3, gy3, z3), _explicit_dz(r1, gy1, z1), NO_LAZY, NO_LAZY)
    got = run(gy3, gy1, dict(r3, z=z3), dict(r1, z=z1))
    for a, b_, what in zip(got, ref, ("dx", "3x3 dW", "1x1 dW")):
        assert torch.isfinite(b_).all()
        _same(a, b_.cpu(), what)
    _check_param_grads(r3)
    _check_param_grads(r1)
