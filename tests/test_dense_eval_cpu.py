"""CPU-side checks of DenseNet's evaluation without concatenations (include/alignq_dense.h): the fifth header's binding, the
refusals that return before anything is launched, the stale-library message, tests/dense_eval_oracle.py against torch, the coverage of
its case table, and the `fuse_dense_eval` flag."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import dense_eval_oracle as DO
from tests import k3conv_exact_oracle as K3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alignq_dense_layer_eval_fwd", "alignq_avgpool2_nhwc_fwd")
vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


# -------------------------------------------------------------------------------------------------------------- the binding
def test_fifth_header_has_its_own_table():
    from alignq_amd import _header, _lib
    want = {"alignq_dense_layer_eval_fwd": (i32, [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, f32, i32, vp]),
            "alignq_avgpool2_nhwc_fwd": (i32, [vp, vp, i32, i32, i32, i32, i32, vp])}
    assert tuple(_lib.DENSE_SIGNATURES) == NAMES
    for name in NAMES:
        got = _lib.DENSE_SIGNATURES[name]
        assert got[0] is want[name][0] and len(got[1]) == len(want[name][1]), name
        assert all(a is b for a, b in zip(got[1], want[name][1])), name
        for table in (_lib.SIGNATURES, _lib.MOBILE_SIGNATURES, _lib.POINTWISE_SIGNATURES, _lib.K3CONV_SIGNATURES):
            assert name not in table
    # the table IS the header: read again here; one record of its own, no constants, and nothing of it in the other four headers
    fns, structs, consts = _header.read(os.path.join(ROOT, "include", "alignq_dense.h"))
    assert fns == _lib.DENSE_SIGNATURES and list(structs) == ["alignq_dense_site"] and consts == {}
    assert [f for f, _ in _lib.DenseSite._fields_] == ["gamma", "beta", "running_mean", "running_var", "bn_eps", "k", "clamp"]
    assert [t for _, t in _lib.DenseSite._fields_] == [vp, vp, vp, vp, f32, i32, i32] and ctypes.sizeof(_lib.DenseSite) == 48
    assert "z" not in dict(_lib.DenseSite._fields_)
    for header in ("alignq.h", "alignq_mobile.h", "alignq_pointwise.h", "alignq_k3conv.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read()
        assert not any(name in text for name in NAMES) and "alignq_dense_site" not in text, header


def test_library_exports_the_dense_symbols():
    from alignq_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is _lib.DENSE_SIGNATURES[name][0] and list(fn.argtypes) == _lib.DENSE_SIGNATURES[name][1]


class _Stale:
    """a stand-in library that answers the ABI version and nothing else"""

    def alignq_abi_version(self):
        from alignq_amd import _lib
        return _lib.ABI_VERSION

    def __getattr__(self, name):
        raise AttributeError(name)


def test_stale_library_without_the_dense_symbols_is_reported(monkeypatch):
    """a libalignq_hip.so built before csrc/dense_eval_kernels.hip existed: AlignQLibraryError that names the header and says to
    rebuild (the four earlier tables are emptied so that load() reaches the fifth)"""
    from alignq_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    for table in ("SIGNATURES", "MOBILE_SIGNATURES", "POINTWISE_SIGNATURES", "K3CONV_SIGNATURES"):
        monkeypatch.setattr(_lib, table, {})
    monkeypatch.setattr(ctypes, "CDLL", lambda path: _Stale())
    with pytest.raises(_lib.AlignQLibraryError, match="alignq_dense.h.*built before.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_the_fifth_table_is_bound_last(monkeypatch):
    """a library that lacks the 3x3 names AND the new ones is reported by the fourth header's message"""
    from alignq_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    for table in ("SIGNATURES", "MOBILE_SIGNATURES", "POINTWISE_SIGNATURES"):
        monkeypatch.setattr(_lib, table, {})
    monkeypatch.setattr(ctypes, "CDLL", lambda path: _Stale())
    with pytest.raises(_lib.AlignQLibraryError, match="alignq_k3conv.h.*rebuild"):
        _lib.load()


def test_the_build_lists_the_new_source_and_headers():
    with open(os.path.join(ROOT, "alignq_amd", "csrc", "Makefile")) as f:
        lines = f.read().split("\n")
    srcs = [ln for ln in lines if ln.startswith("SRCS :=")][0].split()
    deps = [ln for ln in lines if ln.startswith("$(OUT)/%.o:")][0].split()
    assert srcs[-1] == "dense_eval_kernels.hip" and "mobile_eval_kernels.hip" in srcs
    assert "../../include/alignq_dense.h" in deps and "eval_site_body.h" in deps
    # one statement of the site's device functions: both files include the shared header and neither defines them itself
    for src in ("mobile_eval_kernels.hip", "dense_eval_kernels.hip"):
        with open(os.path.join(ROOT, "alignq_amd", "csrc", src)) as f:
            text = f.read()
        assert '#include "eval_site_body.h"' in text
        assert "void ab_table(" not in text and "float4 site_q(" not in text and "float clamp1(" not in text, src


# --------------------------------------------------------------------------------------------------------------- refusals
class Args:
    """valid-looking arguments over GARBAGE pointers (never dereferenced: every refusal returns before a launch)"""
    P16 = 0x10000            # 16-byte aligned, not NULL

    def __init__(self):
        from alignq_amd import _lib
        self.L, self.lib = _lib, _lib.load()

    def rec(self, gamma=P16, beta=P16, mean=P16, var=P16, eps=1e-5, k=4, clamp=1):
        return self.L.DenseSite(gamma, beta, mean, var, eps, k, clamp)

    def layer(self, x=P16, ldx=None, y=P16, ldy=None, rec="ok", w=P16, B=2, H=3, W=3, cin=24, cout=12, w_bit=4, r=2.0, formula=1):
        rec = self.rec() if isinstance(rec, str) else rec
        return self.lib.alignq_dense_layer_eval_fwd(x, cin if ldx is None else ldx, y, cout if ldy is None else ldy,
                                                    None if rec is None else ctypes.byref(rec), w, B, H, W, cin, cout, w_bit, r,
                                                    formula, None)

    def pool(self, x=P16, y=P16, ldy=None, B=2, H=4, W=4, C=12):
        return self.lib.alignq_avgpool2_nhwc_fwd(x, y, C if ldy is None else ldy, B, H, W, C, None)


BAD_C = (0, 2, 6, 10, 13, 516, 2048, -4)


def test_refusals_before_any_launch():
    a = Args()
    EINVAL, EUNSUP = a.L.EINVAL, a.L.EUNSUPPORTED
    P16 = Args.P16
    lim = (1 << 31) - 1
    # ---- alignq_dense_layer_eval_fwd: ALIGNQ_EINVAL
    for n in ("x", "y", "w"):
        assert a.layer(**{n: None}) == EINVAL, n
        for off in (4, 8, 12):
            assert a.layer(**{n: P16 + off}) == EINVAL, (n, off)
    assert a.layer(rec=None) == EINVAL and a.layer(rec=a.rec(mean=None)) == EINVAL and a.layer(rec=a.rec(var=None)) == EINVAL
    for w_bit in (0, 9, 32, -1):
        assert a.layer(w_bit=w_bit) == EINVAL, w_bit
    for k in (0, -1, 17, 31, 33):
        assert a.layer(rec=a.rec(k=k)) == EINVAL, k
    assert a.layer(formula=2) == EINVAL and a.layer(formula=-1) == EINVAL
    assert a.layer(rec=a.rec(clamp=3)) == EINVAL and a.layer(rec=a.rec(clamp=-1)) == EINVAL
    for ld in (23, 20, 0, -24, 26, 25):          # below CIN = 24, or no multiple of 4
        assert a.layer(ldx=ld) == EINVAL, ld
    for ld in (11, 8, 0, -12, 14, 13):
        assert a.layer(ldy=ld) == EINVAL, ld
    # ---- ALIGNQ_EUNSUPPORTED: the shape (pitches that are fine for it)
    for C in BAD_C:
        big = 520 if C < 520 else 2048
        assert a.layer(cin=C, ldx=big) == EUNSUP and a.layer(cout=C, ldy=big) == EUNSUP, C
    for dim in ("B", "H", "W"):
        assert a.layer(**{dim: 0}) == EUNSUP and a.layer(**{dim: -5}) == EUNSUP, dim
    # B * H * W * max(ldx, ldy) <= 2^31 - 1: the PITCH counts, and products beyond 32 and 64 bits are caught
    assert a.layer(B=lim // 512, H=1, W=1, cin=4, ldx=512, w_bit=0) == EINVAL          # (at the limit the shape is fine: never launched here)
    assert a.layer(B=lim // 512 + 1, H=1, W=1, cin=4, ldx=512) == EUNSUP and a.layer(B=1, H=lim // 512 + 1, W=1, cout=4, ldy=512) == EUNSUP
    assert a.layer(B=lim // 24 + 1, H=1, W=1) == EUNSUP
    assert a.layer(B=lim, H=lim, W=lim) == EUNSUP and a.layer(B=1 << 16, H=1 << 16, W=1) == EUNSUP
    # ---- a bad argument is named before an unsupported shape
    assert a.layer(w_bit=0, cin=10, ldx=12) == EINVAL and a.layer(x=None, cout=2, ldy=4) == EINVAL and a.layer(y=P16 + 4, B=0) == EINVAL
    assert a.layer(rec=a.rec(k=0), B=0) == EINVAL and a.layer(formula=5, H=0) == EINVAL and a.layer(rec=a.rec(clamp=7), cin=516, ldx=516) == EINVAL
    assert a.layer(ldx=20, B=0) == EINVAL and a.layer(ldy=13, cin=516) == EINVAL
    # ---- alignq_avgpool2_nhwc_fwd
    for n in ("x", "y"):
        assert a.pool(**{n: None}) == EINVAL and a.pool(**{n: P16 + 4}) == EINVAL and a.pool(**{n: P16 + 8}) == EINVAL, n
    for ld in (8, 11, 13, 14, 0, -12):
        assert a.pool(ldy=ld) == EINVAL, ld
    for C in (0, 2, 6, 13, 2052, 4096, -4):
        assert a.pool(C=C, ldy=4096) == EUNSUP, C
    assert a.pool(H=1) == EUNSUP and a.pool(W=1) == EUNSUP and a.pool(H=0) == EUNSUP and a.pool(B=0) == EUNSUP and a.pool(W=-2) == EUNSUP
    assert a.pool(B=lim // 48 + 1, H=2, W=2) == EUNSUP and a.pool(B=lim, H=lim, W=lim) == EUNSUP
    assert a.pool(B=lim // 2048 + 1, H=2, W=2, C=4, ldy=2048) == EUNSUP          # the output's pitch counts
    assert a.pool(x=None, H=1) == EINVAL and a.pool(ldy=8, B=0) == EINVAL


# ----------------------------------------------------------------------------------------------------------------- oracle
def test_oracle_convolution_and_pool_against_torch():
    rng = np.random.default_rng(5)
    s = rng.standard_normal((2, 5, 7, 12))
    w = rng.standard_normal((8, 12, 3, 3))
    want = torch.nn.functional.conv2d(torch.from_numpy(s).permute(0, 3, 1, 2), torch.from_numpy(w), None, 1, 1).permute(0, 2, 3, 1).numpy()
    assert np.abs(DO.conv3x3_f64(s, w) - want).max() <= 1e-12 * np.abs(want).max()
    for shape in DO.POOL_SHAPES + [(1, 3, 3, 4)]:
        x = (rng.standard_normal(shape) * 3).astype(np.float32)
        got = DO.pool(x)
        want = torch.nn.functional.avg_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
        assert got.shape == want.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3]) and got.dtype == np.float32
        # any order of a four-term fp32 sum: 3 * 2^-24 of the window's mean |x| (the * 0.25 is exact)
        mean_abs = DO.pool(np.abs(x).astype(np.float64).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= 3 * 2.0 ** -24 * mean_abs * (1 + 2.0 ** -20)).all()
    # the stated order, on values where the order shows: ((1 + 2^-24) + 2^-24) + 1 rounds twice to even
    x = np.float32([[[[1.0], [2.0 ** -24]], [[2.0 ** -24], [1.0]]]])
    assert DO.pool(x)[0, 0, 0, 0] == np.float32(0.5)


def test_oracle_layer_pads_with_zeros_behind_the_site():
    """operands keep clamp(q(b_c)) > 0 on every channel, so a padding pixel that went through the site would change the result:
    at a 1 x 1 image the layer is the centre tap alone"""
    for c in DO.CASES:
        if c["grid"] != (1, 1, 1) or c["pitch"] != "contiguous":
            continue
        x, vecs, eps, wq = DO.operands(c)
        s0 = DO.site(np.zeros_like(x), vecs, eps, c["k"], 2.0, c["formula"], c["clamp"])
        assert (s0 > 0).all(), c["id"]
        y = DO.layer(x, vecs, eps, c["k"], 2.0, c["formula"], c["clamp"], wq)
        s = DO.site(x, vecs, eps, c["k"], 2.0, c["formula"], c["clamp"]).astype(np.float64)
        centre = wq[:, :, 1, 1].astype(np.float64) @ s[0, 0, 0]
        assert np.abs(y[0, 0, 0] - centre).max() <= 1e-12 * np.abs(centre).max()          # (fp64 sums in two orders)
        ring = np.broadcast_to(s0, (1, 3, 3, c["cin"])).copy()          # q(b_c) around the image instead of zeros
        ring[0, 1, 1] = s[0, 0, 0]
        wrong = DO.conv3x3_f64(ring, wq)[0, 1, 1]
        assert np.abs(wrong - centre).max() > 1e-3 * np.abs(centre).max()


def test_every_channel_of_every_case_keeps_q_of_b_positive():
    for c in DO.CASES[::7]:
        x, vecs, eps, wq = DO.operands(c)
        s0 = DO.site(np.zeros((1, 1, 1, c["cin"]), np.float32), vecs, eps, c["k"], 2.0, c["formula"], c["clamp"])
        assert (s0 > 0).all(), c["id"]
        n = 2 ** c["w_bit"] - 1
        assert np.array_equal(np.rint(wq * n), np.rint(wq.astype(np.float64) * n)) and np.abs(np.rint(wq * n)).max() <= n


def test_case_table_covers_every_form_and_path():
    from alignq_amd import _lib
    lib = _lib.load()
    assert {(c["cin"], c["cout"]) for c in DO.CASES} == set(DO.CHANNELS) and len({c["id"] for c in DO.CASES}) == len(DO.CASES)
    forms = set()
    for c in DO.CASES:
        B, H, W = c["grid"]
        f = lib.alignq_k3conv_form(K3.K3_FWD, B, H, W, c["cin"], c["cout"])
        assert f == DO.form(c) and f >= 0, c["id"]
        forms.add(f)
        ldx, ldy, off = DO.pitches(c)
        assert ldx % 4 == 0 and ldy % 4 == 0 and ldx >= c["cin"] and ldy >= c["cout"] and B * H * W * max(ldx, ldy) < 2 ** 31
        assert off in (None, c["cin"]) and (off is None or ldx == ldy >= c["cin"] + c["cout"])
    assert forms == K3.FORMS[K3.K3_FWD]                       # every form alignq_k3conv_form returns for the forward
    for cin, cout in DO.CHANNELS:
        mine = [c for c in DO.CASES if (c["cin"], c["cout"]) == (cin, cout)]
        assert {c["grid"] for c in mine} >= set(DO.GRIDS) and {c["pitch"] for c in mine} == set(DO.PITCHES)
        assert {(c["grid"], c["pitch"]) for c in mine} >= {(g, p) for g in DO.GRIDS for p in DO.PITCHES}
        assert {c["k"] for c in mine} == {2, 4, 8, 32} and {c["formula"] for c in mine} == {DO.ADMM, DO.CDF}
        assert {c["clamp"] for c in mine} == {DO.NONE, DO.RELU} and sum(not c["affine"] for c in mine) == 1
    # the chunk structure the pairs were chosen for: one chunk, a tail of 4 and of 28, many chunks
    assert sorted({cin % 32 for cin, _ in DO.CHANNELS}) == [0, 4, 12, 24, 28] and max(cin for cin, _ in DO.CHANNELS) // 32 == 13
    small = [c for c in DO.CASES if (c["cin"], c["cout"]) == (4, 4)]
    big = [c for c in small if c["grid"] == DO.GBIG]
    wt = [c for c in small if c["grid"] == DO.GWT]
    assert len(big) == 3 and len(wt) == 3
    assert all(DO.spatial_tiles(c) > K3.GRID_TILES and DO.write_through(c) for c in big)
    assert all(DO.spatial_tiles(c) <= K3.GRID_TILES and DO.write_through(c) for c in wt)
    B, H, W = DO.GWT
    assert B * H * W * 4 * 4 == DO.WT_MIN_BYTES                               # the first size of the window
    assert not any(DO.write_through(c) for c in DO.CASES if c["grid"] in DO.GRIDS)
    # the tile edges: a grid below, at and beyond one 8 x 8 tile in each direction, and more than one image
    assert {(H % 8, W % 8) for _, H, W in DO.GRIDS} >= {(7, 1), (0, 0), (1, 7)} and any(B > 1 for B, _, _ in DO.GRIDS)


# ------------------------------------------------------------------------------------------------------------------- flag
def test_the_flag_is_declared_on_densenet_only():
    """`fuse_dense_eval` is in paths.FLAGS, declared off on densenet.DenseNet and on no other class; paths.apply / restore set it and
    put it back on the model alone; use_hip_convs sets it only when asked"""
    from alignq_amd import densenet as D
    from alignq_amd import mobilenet as M
    from alignq_amd import paths
    assert "fuse_dense_eval" in paths.FLAGS and paths.FLAGS[-1] == "fuse_dense_eval"
    torch.manual_seed(0)
    net = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    assert D.DenseNet.fuse_dense_eval is False
    declaring = [m for m in net.modules() if hasattr(type(m), "fuse_dense_eval")]
    assert declaring == [net] and "fuse_dense_eval" not in net.__dict__
    rec = paths.apply(net, fuse_dense_eval=True)
    assert len(rec) == 1 and net.fuse_dense_eval is True and not any("fuse_dense_eval" in m.__dict__ for m in net.modules() if m is not net)
    paths.restore(rec)
    assert net.fuse_dense_eval is False and "fuse_dense_eval" not in net.__dict__
    D.use_hip_convs(net)
    assert net.fuse_dense_eval is False and "fuse_dense_eval" not in net.__dict__
    D.use_hip_convs(net, dense_eval=True)
    assert net.fuse_dense_eval is True
    assert not any(hasattr(m, "fuse_dense_eval") for m in M.mobile_v2(4, 4, "second").modules())
    # outside EvalStep's scope the flag changes nothing: forward() takes _forward_eval only inside fused.eval_scope
    from alignq_amd import fused
    assert not fused.eval_active()
