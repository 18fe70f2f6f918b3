"""CPU-side checks of MobileNet-V2's folded evaluation sites (include/alignq_mobile.h): the second header's binding, the refusals
that return before anything is launched, and tests/mobile_eval_oracle.py against torch and against the reference's modules
(fixture G20: tests/golden/gen_goldens_mobilenet_eval.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import mobile_eval_oracle as MO
from tests.conftest import load_golden
from tests.golden.mobilenet_init import REDUCED_CFG, mobilenet_init_

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import eval_inputs as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alignq_site_eval_fwd", "alignq_site_eval_twin_fwd", "alignq_dwconv3x3_site_eval_fwd")
vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float


def test_second_header_has_its_own_table():
    from alignq_amd import _header, _lib
    want = {"alignq_site_eval_fwd": (i32, [vp, i64, i32, f32, i32, vp, vp, vp]),
            "alignq_site_eval_twin_fwd": (i32, [vp, vp, i64, i32, f32, i32, vp, vp]),
            "alignq_dwconv3x3_site_eval_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp])}
    assert tuple(_lib.MOBILE_SIGNATURES) == NAMES
    for name in NAMES:
        got = _lib.MOBILE_SIGNATURES[name]
        assert got[0] is want[name][0] and len(got[1]) == len(want[name][1]), name
        assert all(a is b for a, b in zip(got[1], want[name][1])), name
        assert name not in _lib.SIGNATURES
    assert len(_lib.SIGNATURES) == 149
    # the table IS the header: read again here, and nothing of it is declared in alignq.h
    fns, structs, consts = _header.read(os.path.join(ROOT, "include", "alignq_mobile.h"))
    assert fns == _lib.MOBILE_SIGNATURES and list(structs) == ["alignq_eval_site"]
    assert consts == {"ALIGNQ_CLAMP_NONE": 0, "ALIGNQ_CLAMP_RELU": 1, "ALIGNQ_CLAMP_RELU6": 2}
    assert [f for f, _ in _lib.EvalSite._fields_] == ["z", "gamma", "beta", "running_mean", "running_var", "bn_eps", "k", "clamp"]
    assert ctypes.sizeof(_lib.EvalSite) == 56
    with open(os.path.join(ROOT, "include", "alignq.h")) as f:
        core = f.read()
    assert not any(name in core for name in NAMES) and "alignq_eval_site" not in core


def test_library_exports_the_three_symbols():
    from alignq_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == _lib.MOBILE_SIGNATURES[name][1]
    assert lib.alignq_abi_version() == 23


class Args:
    """valid-looking arguments over GARBAGE pointers (never dereferenced: every refusal returns before a launch)"""
    P16 = 0x10000            # 16-byte aligned, not NULL

    def __init__(self):
        from alignq_amd import _lib
        self.L, self.lib = _lib, _lib.load()

    def rec(self, z=P16, gamma=P16, beta=P16, mean=P16, var=P16, eps=1e-5, k=4, clamp=0):
        return self.L.EvalSite(z, gamma, beta, mean, var, eps, k, clamp)

    def site(self, rec="ok", P=8, C=8, r=2.0, formula=1, res=None, y=P16):
        rec = self.rec() if isinstance(rec, str) else rec
        return self.lib.alignq_site_eval_fwd(None if rec is None else ctypes.byref(rec), P, C, r, formula, res, y, None)

    def twin(self, a="ok", b="ok", P=8, C=8, r=2.0, formula=1, y=P16):
        a = self.rec() if isinstance(a, str) else a
        b = self.rec(clamp=1) if isinstance(b, str) else b
        return self.lib.alignq_site_eval_twin_fwd(None if a is None else ctypes.byref(a), None if b is None else ctypes.byref(b),
                                                  P, C, r, formula, y, None)

    def dw(self, rec="ok", x=P16, w=P16, B=2, H=4, W=4, C=8, s=1, r=2.0, formula=1, y=P16):
        rec = self.rec(z=None) if isinstance(rec, str) else rec
        return self.lib.alignq_dwconv3x3_site_eval_fwd(x, w, None if rec is None else ctypes.byref(rec), B, H, W, C, s, r, formula,
                                                       y, None)


def test_refusals_before_any_launch():
    a = Args()
    EINVAL, EUNSUP = a.L.EINVAL, a.L.EUNSUPPORTED
    P16 = Args.P16
    # ---- alignq_site_eval_fwd
    assert a.site(rec=None) == EINVAL and a.site(y=None) == EINVAL and a.site(P=0) == EINVAL
    assert a.site(rec=a.rec(z=None)) == EINVAL and a.site(rec=a.rec(mean=None)) == EINVAL and a.site(rec=a.rec(var=None)) == EINVAL
    assert a.site(rec=a.rec(z=P16 + 4)) == EINVAL and a.site(y=P16 + 8) == EINVAL and a.site(res=P16 + 4) == EINVAL
    for k in (0, -1, 17, 31, 33):
        assert a.site(rec=a.rec(k=k)) == EINVAL, k
    assert a.site(formula=2) == EINVAL and a.site(formula=-1) == EINVAL
    assert a.site(rec=a.rec(clamp=3)) == EINVAL and a.site(rec=a.rec(clamp=-1)) == EINVAL
    for C in (0, 2, 6, 12 + 1, 2052, 4096):
        assert a.site(C=C) == EUNSUP, C
    assert a.site(rec=a.rec(k=0), C=6) == EINVAL                 # a bad argument is named before an unsupported shape
    # ---- alignq_site_eval_twin_fwd
    assert a.twin(a=None) == EINVAL and a.twin(b=None) == EINVAL and a.twin(y=None) == EINVAL and a.twin(P=-3) == EINVAL
    assert a.twin(a=a.rec(clamp=1)) == EINVAL and a.twin(a=a.rec(clamp=2)) == EINVAL          # nothing follows the sum
    assert a.twin(b=a.rec(z=None)) == EINVAL and a.twin(b=a.rec(z=P16 + 4)) == EINVAL and a.twin(b=a.rec(k=0)) == EINVAL
    assert a.twin(b=a.rec(clamp=5)) == EINVAL and a.twin(formula=7) == EINVAL and a.twin(y=P16 + 4) == EINVAL
    for C in (6, 2052):
        assert a.twin(C=C) == EUNSUP, C
    # ---- alignq_dwconv3x3_site_eval_fwd
    assert a.dw(rec=None) == EINVAL and a.dw(x=None) == EINVAL and a.dw(w=None) == EINVAL and a.dw(y=None) == EINVAL
    assert a.dw(B=0) == EINVAL and a.dw(H=0) == EINVAL and a.dw(W=-1) == EINVAL
    assert a.dw(x=P16 + 4) == EINVAL and a.dw(w=P16 + 8) == EINVAL and a.dw(y=P16 + 12) == EINVAL
    assert a.dw(rec=a.rec(z=None, k=0)) == EINVAL and a.dw(rec=a.rec(z=None, clamp=3)) == EINVAL and a.dw(formula=2) == EINVAL
    assert a.dw(rec=a.rec(z=None, var=None)) == EINVAL
    for C in (6, 2, 2052, 8212):
        assert a.dw(C=C) == EUNSUP, C
    assert a.dw(s=3) == EUNSUP and a.dw(s=0) == EUNSUP
    assert a.dw(B=1 << 10, H=1 << 10, W=1 << 10, C=2048) == EUNSUP          # beyond the depthwise forward's int32 offsets


def test_stale_library_is_reported(monkeypatch):
    """a libalignq_hip.so built before the second header existed: AlignQLibraryError that says to rebuild (a stand-in library
    that exports the ABI version and nothing else; the core table is emptied so that load() reaches the second one)"""
    from alignq_amd import _lib

    class Stale:
        def alignq_abi_version(self):
            return _lib.ABI_VERSION

        def __getattr__(self, name):
            raise AttributeError(name)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SIGNATURES", {})
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(_lib.AlignQLibraryError, match="rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_oracle_relu6_equals_torch_on_finite_inputs():
    rng = np.random.default_rng(20)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 5, np.float32([0.0, 6.0, 5.9999995, 6.0000005, -6.0, 1e-45,
                                                                                      -1e-45, 3e38, -3e38, np.inf, -np.inf])])
    got = MO.clamp(v, MO.RELU6)
    want = torch.nn.ReLU6()(torch.from_numpy(v)).numpy()
    assert np.array_equal(got, want) and got.max() == 6.0 and (got == 6.0).sum() > 100
    assert np.array_equal(MO.clamp(v, MO.RELU), torch.relu(torch.from_numpy(v)).numpy())
    assert MO.clamp(v, MO.NONE) is not None and np.array_equal(MO.bits(MO.clamp(v, MO.NONE)), MO.bits(v))
    # where the conventions differ: NaN and -0 give +0 (torch keeps both)
    odd = MO.clamp(np.float32([np.nan, -0.0]), MO.RELU6)
    assert np.array_equal(MO.bits(odd), np.uint32([0, 0]))
    assert np.array_equal(MO.bits(MO.clamp(np.float32([np.nan, -0.0]), MO.RELU)), np.uint32([0, 0]))


def test_oracle_site_against_the_reference_modules_g20(monkeypatch):
    """G20's teacher-forced site (layers[2]: bn1 -> act_q1 -> ReLU6 of the reference, eval mode) against the oracle: no element
    more than one level from the reference's, at most max(4 n_flip_ref, 8) elements one level off (G17's criterion)."""
    from alignq_amd import mobilenet as M
    g = load_golden("g20_mobilenet_eval")
    monkeypatch.setattr(M.MobileNetV2, "cfg", [tuple(int(v) for v in r) for r in g["cfg_reduced"]])
    assert [tuple(int(v) for v in r) for r in g["cfg_reduced"]] == list(REDUCED_CFG)
    net = mobilenet_init_(M.mobile_v2(int(g["bits"]), int(g["bits"]), str(g["stage"])))
    i = int(g["site_layer"])
    bn = net.layers[i].bn1
    pre = f"buf_layers.{i}.bn1."
    vecs = (bn.weight.detach().numpy(), bn.bias.detach().numpy(), g[pre + "running_mean"], g[pre + "running_var"])
    k, r = int(g["bits"]), float(g["act_range"])
    z = np.ascontiguousarray(g["site_z"].transpose(0, 2, 3, 1))
    xq = MO.quant(MO.affine(z, *vecs, float(g["site_bn_eps"])), k, r, MO.CDF)
    ref_xq = np.ascontiguousarray(g["site_xq"].transpose(0, 2, 3, 1))
    d = np.abs(E.levels(xq, k, r, "cdf") - E.levels(ref_xq, k, r, "cdf"))
    n_flip_ref = int(g["site_n_flip_ref"])
    print("G20 site: %d of %d elements one level off (n_flip_ref %d), max %d" % (int((d == 1).sum()), d.size, n_flip_ref, int(d.max())))
    assert d.max() <= 1
    assert int((d == 1).sum()) <= max(4 * n_flip_ref, 8)
    y = MO.finish(xq, MO.RELU6)
    ref_y = np.ascontiguousarray(g["site_y"].transpose(0, 2, 3, 1))
    same = d == 0
    assert np.abs(y[same] - ref_y[same]).max() <= 2.0 ** -22 * r          # the same level: the level value to an ulp of act_range
    assert (ref_y > 0).mean() > 0.2 and len(np.unique(ref_y)) >= 4


def test_g20_targets_keep_their_margin():
    g = load_golden("g20_mobilenet_eval")
    lg, y = g["logits"], g["targets"]
    m = E.margins(lg, y).min(axis=1)
    span = lg.max(axis=1) - lg.min(axis=1)
    assert (m >= float(g["margin_fraction"]) * span).all() and float(g["margin_fraction"]) == 0.05
    assert m.min() >= float(g["min_margin"]) - 1e-6 and float(g["min_margin"]) > 0.1          # (the generator also keeps ranks 4 AND 5 away)
    ce, n1, n5, n = E.metrics_numpy(lg, y)
    assert (n1, n5, n) == (round(float(g["prec1"]) * n / 100), round(float(g["prec5"]) * n / 100), int(g["batch"]))
    assert 0 < n1 < n5 < n                                        # hits, top-5-only hits and misses are all present
    assert abs(ce / n - float(g["ce"])) < 1e-5
