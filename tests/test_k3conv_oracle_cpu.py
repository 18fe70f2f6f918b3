"""CPU-side checks of the 3x3 convolutions at any multiple of 4 channels (include/alignq_k3conv.h): every row of
tests/k3conv_exact_oracle.py keeps the 2^24 budget and holds the operand classes it claims, the table reaches every launch form the
library can choose, the fourth header has a table of its own that is bound last, and every refusal returns before anything is
launched."""
import ctypes
import os

import pytest
import torch

from tests import k3conv_exact_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alignq_k3conv_supported", "alignq_k3conv_form", "alignq_k3conv_fwd", "alignq_k3conv_dgrad", "alignq_k3conv_wgrad_ws_bytes",
         "alignq_k3conv_wgrad")
vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("c", O.G_CASES, ids=_ids(O.G_CASES))
def test_forward_and_data_gradient_rows_keep_the_budget_and_their_classes(c):
    a, b = O.g_operands(c)
    worst = O.g_budget(c, a, b)
    assert 0 < worst < O.TWO24
    assert int(b.abs().max()) <= O.nlev_of(c) and tuple(b.shape) == (c["cout"], 3, 3, c["cin"])
    f2, f3 = O.class_fractions(a)
    if c["set"] == "dense":
        assert (f2, f3) == (0.0, 0.0) and int(a.abs().max()) <= 255          # class 1: one bf16 term
    else:
        assert f2 == 1.0 and f3 > 0.3                                        # class 3: all three terms carry value
        # every (output, tap) contraction meets a non-zero bin: no tap is trivially absent
        assert bool((b.abs().sum(dim=3 if c["op"] == "fwd" else 0) > 0).all())


@pytest.mark.parametrize("c", O.ALL_WGRAD, ids=_ids(O.ALL_WGRAD))
def test_filter_gradient_rows_keep_the_budget_and_their_classes(c):
    x, dy = O.wgrad_operands(c)
    worst = O.assert_exact_budget(O.wgrad_i64, x, dy, ks=3, stride=1, pad=1)
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
    # the sparse pixels: image corners, the last pixel, both sides of a step boundary each way, every 4-pixel block of a step
    assert O.wgrad_steps(c) == 18
    for co in (0, c["cout"] - 1):
        px = O.wgrad_pixels(c, co)
        assert {(0, 0, 0), (c["B"] - 1, c["h"] - 1, c["w"] - 1), (0, 1, 7), (0, 1, 8), (0, 3, 2), (0, 4, 2)} <= set(px)
        assert {(8 * h + w) // 4 for b, h, w in px if b == 1} == set(range(8))
        assert all(int(dy[b, h, w, co]) != 0 for b, h, w in px) and int((dy[..., co] != 0).sum()) == O.SPARSE_K


def test_pair_rows_cover_the_pairs_the_header_takes():
    """(dy, x) classes (1,3), (3,1), (2,2): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1 - the six pairs of the header - at
    both filter-gradient forms"""
    from tests.conv_exact_oracle import PAIR_CLASSES
    assert O.PAIR_CLASSES == PAIR_CLASSES
    assert {(c["form"], c["set"]) for c in O.WGRAD_PAIRS} == {(f, "dy%d_x%d" % p) for f in O.FORMS[O.K3_WGRAD] for p in PAIR_CLASSES}
    with open(os.path.join(ROOT, "include", "alignq_k3conv.h")) as f:
        text = f.read()
    assert "(x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0)" in text


def test_table_reaches_every_launch_form_and_every_edge():
    """alignq_k3conv_form over every supported channel pair (it needs no GPU): the values it returns are the table's FORMS, each row's
    form is what the library answers, the rows cover every form of every operation, and the workspace query follows the slab rule"""
    from alignq_amd import _lib
    lib = _lib.load()
    seen = {op: set() for op in O.FORMS}
    for cin in range(4, 513, 4):
        for cout in (4, 12, 24, 36, 64, 444, 512):
            for op in O.FORMS:
                seen[op].add(lib.alignq_k3conv_form(op, 3, 5, 5, cin, cout))
                seen[op].add(lib.alignq_k3conv_form(op, 3, 5, 5, cout, cin))
    assert seen == O.FORMS
    for op, name, rows in ((O.K3_FWD, "fwd", O.FWD), (O.K3_DGRAD, "dgrad", O.DGRAD), (O.K3_WGRAD, "wgrad", O.ALL_WGRAD)):
        assert {c["form"] for c in rows} == O.FORMS[op], name
        for c in rows:
            g = (c["B"], c["h"], c["w"], c["cin"], c["cout"])
            assert lib.alignq_k3conv_supported(*g) == 1 and lib.alignq_k3conv_form(op, *g) == c["form"], c["id"]
            if name == "wgrad":
                n_slabs, per = O.wgrad_slabs(c)
                assert (n_slabs - 1) * per < O.wgrad_steps(c) <= n_slabs * per, c["id"]          # no slab is empty
                assert lib.alignq_k3conv_wgrad_ws_bytes(*g) == n_slabs * 4 * 9 * c["cin"] * c["cout"], c["id"]
    assert lib.alignq_k3conv_form(3, 3, 5, 5, 12, 12) == -1 and lib.alignq_k3conv_form(-1, 3, 5, 5, 12, 12) == -1
    assert lib.alignq_k3conv_form(O.K3_FWD, 3, 5, 5, 10, 12) == -1 and lib.alignq_k3conv_form(O.K3_FWD, 0, 5, 5, 12, 12) == -1
    # the N = 12 tile wastes one quarter of 16 channels, not more
    assert lib.alignq_k3conv_form(O.K3_FWD, 128, 32, 32, 24, 12) == 0 and lib.alignq_k3conv_form(O.K3_DGRAD, 128, 8, 8, 444, 12) == 2
    # spot values of the slab rule
    by_id = {c["id"]: c for c in O.ALL_WGRAD}
    assert O.wgrad_slabs(by_id["wgrad_24x12_B1H1W1_dense"]) == (1, 1) and O.wgrad_slabs(by_id["wgrad_24x12_B3H9W9_dense"]) == (9, 2)
    assert O.wgrad_slabs(by_id["wgrad_4x4_B16H64W64_dense"]) == (512, 4) and O.wgrad_slabs(by_id["wgrad_444x12_B3H5W5_dense"]) == (3, 2)
    assert O.wgrad_channel_tiles(by_id["wgrad_12x444_B3H5W5_dense"]) == 7 and O.wgrad_channel_tiles(by_id["wgrad_512x4_B3H5W5_dense"]) == 8
    # the grid-stride case lies beyond one pass of the grid cap and the write-through case inside one pass; both inside the window,
    # every other row below it
    big, wt = by_id_g("fwd_4x4_B33H64W64_dense"), by_id_g("fwd_4x4_B16H64W64_dense")
    assert O.grid_tiles(big) > O.GRID_TILES >= O.grid_tiles(wt)
    for c in O.G_CASES:
        nbytes = 4 * O.rows_of(c) * (c["cout"] if c["op"] == "fwd" else c["cin"])
        assert ((1 << 20) <= nbytes <= (64 << 20)) == ((c["B"], c["h"], c["w"]) in (O.GBIG, O.GWT)), c["id"]
    # the spatial edges: one pixel, one row, one column, B > 1, and tile - 1, tile, tile + 1 each way
    for rows, th, tw in ((O.FWD, O.TILE, O.TILE), (O.DGRAD, O.TILE, O.TILE), (O.ALL_WGRAD, O.STEP_H, O.STEP_W)):
        hs, ws = {c["h"] for c in rows if c["B"] == 1}, {c["w"] for c in rows if c["B"] == 1}
        assert {1, th - 1, th, th + 1} <= hs and {1, tw - 1, tw, tw + 1} <= ws
        assert {(2, 1, 5), (2, 5, 1), (3, 5, 5)} <= {(c["B"], c["h"], c["w"]) for c in rows}
        assert sum(c["set"] != "dense" for c in rows) >= 5


def by_id_g(cid):
    return {c["id"]: c for c in O.G_CASES}[cid]


# -------------------------------------------------------------------------------------------------------------- the binding
def test_fourth_header_has_its_own_table():
    from alignq_amd import _header, _lib
    geom = [i32] * 5
    want = {"alignq_k3conv_supported": (i32, geom),
            "alignq_k3conv_form": (i32, [i32] + geom),
            "alignq_k3conv_fwd": (i32, [vp, vp, vp] + geom + [i32, vp]),
            "alignq_k3conv_dgrad": (i32, [vp, vp, vp] + geom + [i32, vp]),
            "alignq_k3conv_wgrad_ws_bytes": (sz, geom),
            "alignq_k3conv_wgrad": (i32, [vp, vp, vp, vp] + geom + [vp, vp])}
    assert tuple(_lib.K3CONV_SIGNATURES) == NAMES
    for name in NAMES:
        got = _lib.K3CONV_SIGNATURES[name]
        assert got[0] is want[name][0] and len(got[1]) == len(want[name][1]), name
        assert all(a is b for a, b in zip(got[1], want[name][1])), name
        assert name not in _lib.SIGNATURES and name not in _lib.MOBILE_SIGNATURES and name not in _lib.POINTWISE_SIGNATURES
    assert len(_lib.SIGNATURES) == 149 and len(_lib.MOBILE_SIGNATURES) == 3 and len(_lib.POINTWISE_SIGNATURES) == 6
    assert _lib.ABI_VERSION == 23
    fns, structs, consts = _header.read(os.path.join(ROOT, "include", "alignq_k3conv.h"))
    assert fns == _lib.K3CONV_SIGNATURES and not structs
    assert (consts["ALIGNQ_K3_FWD"], consts["ALIGNQ_K3_DGRAD"], consts["ALIGNQ_K3_WGRAD"]) == (O.K3_FWD, O.K3_DGRAD, O.K3_WGRAD)
    assert (_lib.K3_FWD, _lib.K3_DGRAD, _lib.K3_WGRAD) == (O.K3_FWD, O.K3_DGRAD, O.K3_WGRAD)
    # the table covers every form constant of the header
    assert {v for k, v in consts.items() if k.startswith("ALIGNQ_K3_FORM_N")} == O.FORMS[O.K3_FWD] == O.FORMS[O.K3_DGRAD]
    assert {v for k, v in consts.items() if k.startswith("ALIGNQ_K3_FORM_W")} == O.FORMS[O.K3_WGRAD]
    assert len([k for k in consts if k.startswith("ALIGNQ_K3_FORM_")]) == 5
    for header in ("alignq.h", "alignq_mobile.h", "alignq_pointwise.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read()
        assert not any(name in text for name in NAMES), header


def test_library_exports_the_k3conv_symbols():
    from alignq_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is _lib.K3CONV_SIGNATURES[name][0] and list(fn.argtypes) == _lib.K3CONV_SIGNATURES[name][1]
    assert lib.alignq_abi_version() == 23


def test_stale_library_without_the_k3conv_symbols_is_reported(monkeypatch):
    """a libalignq_hip.so built before csrc/k3conv_kernels.hip existed: AlignQLibraryError that names the header and says to rebuild
    (a stand-in that answers everything but the new names; the three earlier tables are emptied)"""
    from alignq_amd import _lib

    class Stale:
        def alignq_abi_version(self):
            return _lib.ABI_VERSION

        def __getattr__(self, name):
            raise AttributeError(name)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SIGNATURES", {})
    monkeypatch.setattr(_lib, "MOBILE_SIGNATURES", {})
    monkeypatch.setattr(_lib, "POINTWISE_SIGNATURES", {})
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(_lib.AlignQLibraryError, match="alignq_k3conv.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_the_earlier_tables_are_bound_first(monkeypatch):
    """a library that lacks the pointwise AND the new names is reported by the pointwise header's message: the new table is bound last"""
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


# --------------------------------------------------------------------------------------------------------------- refusals
class Args:
    """valid-looking arguments over GARBAGE pointers (never dereferenced: every refusal returns before a launch)"""
    P16 = 0x10000            # 16-byte aligned, not NULL

    def __init__(self):
        from alignq_amd import _lib
        self.L, self.lib = _lib, _lib.load()

    def fwd(self, x=P16, w=P16, y=P16, B=2, H=3, W=3, cin=12, cout=12, k=4):
        return self.lib.alignq_k3conv_fwd(x, w, y, B, H, W, cin, cout, k, None)

    def dgrad(self, dy=P16, w=P16, dx=P16, B=2, H=3, W=3, cin=12, cout=12, k=4):
        return self.lib.alignq_k3conv_dgrad(dy, w, dx, B, H, W, cin, cout, k, None)

    def wgrad(self, x=P16, dy=P16, dw=P16, ws=P16, B=2, H=3, W=3, cin=12, cout=12, ns=None):
        return self.lib.alignq_k3conv_wgrad(x, dy, dw, ws, B, H, W, cin, cout, ns, None)


BAD_C = (0, 2, 6, 10, 13, 516, 2048, -4)


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
        for k in (0, 9, 32, -1):
            assert call(k=k) == EINVAL, k
        for C in BAD_C:
            assert call(cin=C) == EUNSUP and call(cout=C) == EUNSUP, C
        for dim in ("B", "H", "W"):
            assert call(**{dim: 0}) == EUNSUP and call(**{dim: -5}) == EUNSUP, dim
        # the int32 offset limit: B * H * W * max(CIN, COUT) <= 2^31 - 1, also where B * H * W alone overflows 32 or 64 bits
        assert call(B=lim // 512 + 1, H=1, W=1, cin=512) == EUNSUP and call(B=1, H=lim // 512 + 1, W=1, cout=512) == EUNSUP
        assert call(B=lim // 512, H=1, W=1, cin=512, k=0) == EINVAL
        assert call(B=lim, H=lim, W=lim) == EUNSUP and call(B=1 << 16, H=1 << 16, W=1) == EUNSUP
        # a bad argument is named before an unsupported shape
        assert call(k=0, cin=10) == EINVAL and call(**{names[0]: None}, cout=2) == EINVAL and call(**{names[2]: P16 + 4}, B=0) == EINVAL
    ns = ctypes.c_int(0)
    for n in ("x", "dy", "ws"):
        assert a.wgrad(**{n: None}) == EINVAL and a.wgrad(**{n: P16 + 8}) == EINVAL, n
    assert a.wgrad(dw=None) == EINVAL                      # neither a gradient nor a slab count to report
    assert a.wgrad(dw=P16 + 4) == EINVAL and a.wgrad(dw=P16 + 4, ns=ctypes.byref(ns)) == EINVAL
    for C in BAD_C:
        assert a.wgrad(cin=C) == EUNSUP and a.wgrad(cout=C) == EUNSUP, C
        assert a.wgrad(dw=None, ns=ctypes.byref(ns), cin=C) == EUNSUP      # the deferred form: dw may be NULL, the shape still counts
    assert a.wgrad(B=0) == EUNSUP and a.wgrad(B=lim // 512 + 1, H=1, W=1, cout=512) == EUNSUP
    assert a.wgrad(x=None, cin=10) == EINVAL and ns.value == 0
    # the queries answer the same set
    assert a.lib.alignq_k3conv_supported(lim // 512, 1, 1, 512, 4) == 1 and a.lib.alignq_k3conv_supported(lim // 512 + 1, 1, 1, 512, 4) == 0
    assert a.lib.alignq_k3conv_supported(1, 1, 1, 4, 4) == 1 and a.lib.alignq_k3conv_supported(1, 0, 1, 4, 4) == 0
    assert a.lib.alignq_k3conv_supported(128, 32, 32, 24, 12) == 1 and a.lib.alignq_k3conv_supported(128, 8, 8, 444, 12) == 1
    for C in BAD_C:
        assert a.lib.alignq_k3conv_supported(2, 3, 3, C, 12) == 0 and a.lib.alignq_k3conv_supported(2, 3, 3, 12, C) == 0
        assert a.lib.alignq_k3conv_wgrad_ws_bytes(2, 3, 3, C, 12) == 0
    # the other convolutions keep their sets
    assert a.lib.alignq_qconv_supported(2, 8, 8, 24, 12, 3, 1) == 0 and a.lib.alignq_pwconv_supported(8, 12, 12) == 0


def test_the_flag_is_declared_on_densenets_class_only():
    """`use_qconv_k3` is in paths.FLAGS, declared off by densenet's convolution class and by no class of the other models;
    use_hip_convs sets it on exactly the 3x3 modules"""
    from alignq_amd import densenet as D
    from alignq_amd import mobilenet as M
    from alignq_amd import paths
    assert "use_qconv_k3" in paths.FLAGS
    torch.manual_seed(0)
    net = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    k3 = [m for m in net.modules() if hasattr(type(m), "use_qconv_k3")]
    assert len(k3) == 7 and all(type(m).__name__ == "Conv2d_Q3" and m.kernel_size == (3, 3) for m in k3)
    assert all(m.use_qconv_k3 is False and "use_qconv_k3" not in m.__dict__ for m in k3)
    D.use_hip_convs(net)
    assert all(m.use_qconv_k3 is True and m.use_qconv is True for m in k3)
    assert not any(hasattr(m, "use_qconv_k3") for m in M.mobile_v2(4, 4, "second").modules())
