"""CPU-side checks of the pointwise convolutions (include/alignq_pointwise.h): every row of tests/pointwise_exact_oracle.py keeps
the 2^24 budget and holds the operand classes it claims, the table reaches every launch form the library can choose, the third
header has a table of its own, and every refusal returns before anything is launched."""
import ctypes
import os

import pytest
import torch

from tests import pointwise_exact_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alignq_pwconv_supported", "alignq_pwconv_form", "alignq_pwconv_fwd", "alignq_pwconv_dgrad", "alignq_pwconv_wgrad_ws_bytes",
         "alignq_pwconv_wgrad")
vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t


def _ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("c", O.G_CASES, ids=_ids(O.G_CASES))
def test_forward_and_data_gradient_rows_keep_the_budget_and_their_classes(c):
    a, b = O.g_operands(c)
    worst = O.g_budget(c, a, b)
    assert 0 < worst < O.TWO24
    assert int(b.abs().max()) <= 255 and tuple(b.shape) == (c["cout"], 1, 1, c["cin"])
    f2, f3 = O.class_fractions(a)
    if c["set"] == "dense":
        assert (f2, f3) == (0.0, 0.0) and int(a.abs().max()) <= 255          # class 1: one bf16 term
    else:
        assert f2 == 1.0 and f3 > 0.3                                        # class 3: all three terms carry value
        # every contraction meets a non-zero bin: no output is trivially zero
        assert bool((b.abs().sum(dim=3 if c["op"] == "fwd" else 0) > 0).all())


@pytest.mark.parametrize("c", O.ALL_WGRAD, ids=_ids(O.ALL_WGRAD))
def test_filter_gradient_rows_keep_the_budget_and_their_classes(c):
    x, dy = O.wgrad_operands(c)
    worst = O.assert_exact_budget(O.wgrad_i64, x, dy, ks=1, stride=1, pad=0)
    assert 0 < worst < O.TWO24
    if c["set"] == "dense":
        assert O.class_fractions(x) == (0.0, 0.0) and O.class_fractions(dy) == (0.0, 0.0)
        return
    want = {1: (0.0, 0.0), 2: (1.0, 0.0)}
    for t, cls in ((dy, int(c["set"][2])), (x, int(c["set"][5]))):
        f2, f3 = O.class_fractions(t)
        if cls == 3:
            assert f2 == 1.0 and f3 > 0.3
        else:
            assert (f2, f3) == want[cls]
    # the sparse pixels: first, last, both sides of the step and of the slab boundary, every 4-pixel row block of a step
    n_slabs, per = O.wgrad_slabs(c)
    assert n_slabs == 3 and per == 64
    for co in (0, c["cout"] - 1):
        px = set(O.wgrad_pixels(c, co))
        assert {0, O.rows_of(c) - 1, 31, 32, per - 1, per} <= px
        assert {(p - per) // 4 for p in px if per <= p < per + 32} == set(range(8))
        assert bool((dy.reshape(-1, c["cout"])[sorted(px), co] != 0).all())


def test_pair_rows_cover_the_pairs_the_header_takes():
    """(dy, x) classes (1,3), (3,1), (2,2): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1 - the six pairs of the header - at one
    shape per filter-gradient form"""
    from tests.conv_exact_oracle import PAIR_CLASSES
    assert O.PAIR_CLASSES == PAIR_CLASSES
    assert {(c["form"], c["set"]) for c in O.WGRAD_PAIRS} == {(f, "dy%d_x%d" % p) for f in O.FORMS[O.PW_WGRAD] for p in PAIR_CLASSES}
    with open(os.path.join(ROOT, "include", "alignq_pointwise.h")) as f:
        text = f.read()
    assert "(x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0)" in text


def test_table_reaches_every_launch_form():
    """alignq_pwconv_form over every supported channel pair (it needs no GPU): the values it returns are the table's FORMS, each
    row's form is what the library answers, and the rows cover every form of every operation"""
    from alignq_amd import _lib
    lib = _lib.load()
    widths = range(8, 2049, 8)
    seen = {op: set() for op in O.FORMS}
    for cin in widths:
        for cout in (8, 16, 24, 32, 40, 64, 96, 144, 160, 200, 320, 2048):
            for op in O.FORMS:
                seen[op].add(lib.alignq_pwconv_form(op, 75, cin, cout))
                seen[op].add(lib.alignq_pwconv_form(op, 75, cout, cin))
    assert seen == O.FORMS
    for op, name, rows in ((O.PW_FWD, "fwd", O.FWD), (O.PW_DGRAD, "dgrad", O.DGRAD), (O.PW_WGRAD, "wgrad", O.ALL_WGRAD)):
        assert {c["form"] for c in rows} == O.FORMS[op], name
        for c in rows:
            assert lib.alignq_pwconv_form(op, O.rows_of(c), c["cin"], c["cout"]) == c["form"], c["id"]
            if name == "wgrad":
                n_slabs, _ = O.wgrad_slabs(c)
                assert lib.alignq_pwconv_wgrad_ws_bytes(O.rows_of(c), c["cin"], c["cout"]) == n_slabs * 4 * c["cin"] * c["cout"], c["id"]
    assert lib.alignq_pwconv_form(3, 75, 8, 8) == -1 and lib.alignq_pwconv_form(-1, 75, 8, 8) == -1
    assert lib.alignq_pwconv_form(O.PW_FWD, 75, 12, 8) == -1 and lib.alignq_pwconv_form(O.PW_FWD, 0, 8, 8) == -1
    # spot values of the slab rule: 75 pixels = two slabs of 64; the big case = 512 slabs of 288 pixels, the last 56 empty
    by_id = {c["id"]: c for c in O.ALL_WGRAD}
    assert O.wgrad_slabs(by_id["wgrad_8x8_M75_dense"]) == (2, 64) and O.wgrad_slabs(by_id["wgrad_8x8_M1_dense"]) == (1, 32)
    assert O.wgrad_slabs(by_id["wgrad_8x8_M131143_dense"]) == (512, 288) and 456 * 288 > 131143 > 455 * 288
    assert O.wgrad_slabs(by_id["wgrad_2048x8_M189_dense"]) == (3, 64) and O.wgrad_tiles(by_id["wgrad_40x200_M189_dense"]) == 4
    # the grid-stride case lies beyond one pass of the grid cap, the others inside it
    big = O.rows_of(by_id["wgrad_8x8_M131143_dense"])
    assert -(-big // O.TILE_ROWS) > O.GRID_ROW_TILES and 1 << 20 <= big * 8 * 4 <= 64 << 20


# -------------------------------------------------------------------------------------------------------------- the binding
def test_third_header_has_its_own_table():
    from alignq_amd import _header, _lib
    want = {"alignq_pwconv_supported": (i32, [i64, i32, i32]),
            "alignq_pwconv_form": (i32, [i32, i64, i32, i32]),
            "alignq_pwconv_fwd": (i32, [vp, vp, vp, i64, i32, i32, i32, vp]),
            "alignq_pwconv_dgrad": (i32, [vp, vp, vp, i64, i32, i32, i32, vp]),
            "alignq_pwconv_wgrad_ws_bytes": (sz, [i64, i32, i32]),
            "alignq_pwconv_wgrad": (i32, [vp, vp, vp, vp, i64, i32, i32, vp, vp])}
    assert tuple(_lib.POINTWISE_SIGNATURES) == NAMES
    for name in NAMES:
        got = _lib.POINTWISE_SIGNATURES[name]
        assert got[0] is want[name][0] and len(got[1]) == len(want[name][1]), name
        assert all(a is b for a, b in zip(got[1], want[name][1])), name
        assert name not in _lib.SIGNATURES and name not in _lib.MOBILE_SIGNATURES
    assert len(_lib.SIGNATURES) == 149 and len(_lib.MOBILE_SIGNATURES) == 3
    fns, structs, consts = _header.read(os.path.join(ROOT, "include", "alignq_pointwise.h"))
    assert fns == _lib.POINTWISE_SIGNATURES and not structs
    assert (consts["ALIGNQ_PW_FWD"], consts["ALIGNQ_PW_DGRAD"], consts["ALIGNQ_PW_WGRAD"]) == (O.PW_FWD, O.PW_DGRAD, O.PW_WGRAD)
    assert {v for k, v in consts.items() if k.startswith("ALIGNQ_PW_FORM_N")} == O.FORMS[O.PW_FWD]
    assert {v for k, v in consts.items() if k.startswith("ALIGNQ_PW_FORM_W")} == O.FORMS[O.PW_WGRAD]
    for header in ("alignq.h", "alignq_mobile.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read()
        assert not any(name in text for name in NAMES), header


def test_library_exports_the_pointwise_symbols():
    from alignq_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is _lib.POINTWISE_SIGNATURES[name][0] and list(fn.argtypes) == _lib.POINTWISE_SIGNATURES[name][1]
    assert lib.alignq_abi_version() == 23


def test_stale_library_without_the_pointwise_symbols_is_reported(monkeypatch):
    """a libalignq_hip.so built before csrc/pointwise_kernels.hip existed: AlignQLibraryError that names the header and says to
    rebuild (a stand-in that answers everything but the pointwise names; the two earlier tables are emptied)"""
    from alignq_amd import _lib

    class Stale:
        def alignq_abi_version(self):
            return _lib.ABI_VERSION

        def __getattr__(self, name):
            raise AttributeError(name)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SIGNATURES", {})
    monkeypatch.setattr(_lib, "MOBILE_SIGNATURES", {})
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(_lib.AlignQLibraryError, match="alignq_pointwise.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


# --------------------------------------------------------------------------------------------------------------- refusals
class Args:
    """valid-looking arguments over GARBAGE pointers (never dereferenced: every refusal returns before a launch)"""
    P16 = 0x10000            # 16-byte aligned, not NULL

    def __init__(self):
        from alignq_amd import _lib
        self.L, self.lib = _lib, _lib.load()

    def fwd(self, x=P16, w=P16, y=P16, M=8, cin=8, cout=8, k=4):
        return self.lib.alignq_pwconv_fwd(x, w, y, M, cin, cout, k, None)

    def dgrad(self, dy=P16, w=P16, dx=P16, M=8, cin=8, cout=8, k=4):
        return self.lib.alignq_pwconv_dgrad(dy, w, dx, M, cin, cout, k, None)

    def wgrad(self, x=P16, dy=P16, dw=P16, ws=P16, M=8, cin=8, cout=8, ns=None):
        return self.lib.alignq_pwconv_wgrad(x, dy, dw, ws, M, cin, cout, ns, None)


def test_refusals_before_any_launch():
    a = Args()
    EINVAL, EUNSUP = a.L.EINVAL, a.L.EUNSUPPORTED
    P16 = Args.P16
    lim = (1 << 31) - 1
    for call, names in ((a.fwd, ("x", "w", "y")), (a.dgrad, ("dy", "w", "dx"))):
        for n in names:
            assert call(**{n: None}) == EINVAL, n
            for off in (4, 8, 12):
                assert call(**{n: P16 + off}) == EINVAL, (n, off)
        for k in (0, 9, -1):
            assert call(k=k) == EINVAL, k
        for C in (0, 4, 12, 20, 2056, -8):
            assert call(cin=C) == EUNSUP and call(cout=C) == EUNSUP, C
        assert call(M=0) == EUNSUP and call(M=-5) == EUNSUP
        # the int32 offset limit: M * max(CIN, COUT) <= 2^31 - 1
        assert call(M=lim // 2048 + 1, cin=2048) == EUNSUP and call(M=lim // 2048 + 1, cout=2048) == EUNSUP
        assert call(M=1 << 40) == EUNSUP
        # a bad argument is named before an unsupported shape
        assert call(k=0, cin=12) == EINVAL and call(**{names[0]: None}, cout=4) == EINVAL and call(**{names[2]: P16 + 4}, M=0) == EINVAL
    ns = ctypes.c_int(0)
    for n in ("x", "dy", "ws"):
        assert a.wgrad(**{n: None}) == EINVAL and a.wgrad(**{n: P16 + 8}) == EINVAL, n
    assert a.wgrad(dw=None) == EINVAL                      # neither a gradient nor a slab count to report
    assert a.wgrad(dw=P16 + 4) == EINVAL and a.wgrad(dw=P16 + 4, ns=ctypes.byref(ns)) == EINVAL
    for C in (0, 4, 12, 20, 2056):
        assert a.wgrad(cin=C) == EUNSUP and a.wgrad(cout=C) == EUNSUP, C
        assert a.wgrad(dw=None, ns=ctypes.byref(ns), cin=C) == EUNSUP      # the deferred form: dw may be NULL, the shape still counts
    assert a.wgrad(M=0) == EUNSUP and a.wgrad(M=lim // 2048 + 1, cout=2048) == EUNSUP
    assert a.wgrad(x=None, cin=12) == EINVAL and ns.value == 0
    # the queries answer the same set
    assert a.lib.alignq_pwconv_supported(lim // 2048, 2048, 8) == 1 and a.lib.alignq_pwconv_supported(lim // 2048 + 1, 2048, 8) == 0
    assert a.lib.alignq_pwconv_supported(1, 8, 8) == 1 and a.lib.alignq_pwconv_supported(0, 8, 8) == 0
    for C in (0, 4, 12, 20, 2056):
        assert a.lib.alignq_pwconv_supported(8, C, 8) == 0 and a.lib.alignq_pwconv_supported(8, 8, C) == 0
        assert a.lib.alignq_pwconv_wgrad_ws_bytes(8, C, 8) == 0
    # alignq_qconv_* keeps its set (tests/test_gpu_qconv.py pins the same refusal on the GPU machine)
    assert a.lib.alignq_qconv_supported(2, 8, 8, 48, 64, 1, 1) == 0


def test_default_is_off_and_the_opt_in_sets_one_attribute():
    """mobilenet.use_hip_convs(model) leaves `use_qconv_pw` at Conv2d_Q's class default, off, in no instance and on no other kind of
    module; pointwise=True sets it on every Conv2d_Q"""
    from alignq_amd import mobilenet as M
    torch.manual_seed(0)
    net = M.use_hip_convs(M.mobile_v2(4, 4, "second"))
    convs = [m for m in net.modules() if hasattr(m, "quantize_fn")]
    assert convs and all(m.use_qconv for m in convs)
    assert all(m.use_qconv_pw is False and "use_qconv_pw" not in m.__dict__ for m in convs)
    assert not any(hasattr(m, "use_qconv_pw") for m in net.modules() if not hasattr(m, "quantize_fn"))
    net = M.use_hip_convs(net, pointwise=True)
    assert all(m.use_qconv_pw is True for m in convs)
    assert not any(hasattr(m, "use_qconv_pw") for m in net.modules() if not hasattr(m, "quantize_fn"))
